/*
 * graphop_hip.h -- C ABI of the MI355X (gfx950) graph-attention operator library
 *                  (libgraphop_hip.so, built from custom_op_benchmark_amd/csrc/).
 *
 * This is the drop-in boundary for the reference's hot path.  The reference exposes the
 * path as a pybind11 module `graphop` with eight functions on at::Tensor
 * (graphop/graphop.cpp:216-225).  Each entry point below replaces one of them, with the
 * tensors flattened to plain device pointers + sizes; a binding (ctypes / pybind / cgo ...)
 * recovers the reference signature exactly -- see INTEGRATION.md and
 * custom_op_benchmark_amd/graphop.py (the Python binding shipped here).
 *
 * Conventions (all entry points)
 *   - every pointer is a DEVICE pointer (hipMalloc / torch CUDA tensor storage), contiguous,
 *     row-major; index arrays are int64 exactly as in the reference
 *     (graphop_kernel.cu:293-296); value arrays are `dtype` (GRAPHOP_F32 / GRAPHOP_F64, the
 *     reference's AT_DISPATCH_FLOATING_TYPES set, graphop_kernel.cu:291).
 *   - chunked CSR: row[n_chunks], indptr[n_chunks+1] as produced by partition_csr
 *     (part_csr.py:13-27); eid[n_edges], indices[n_edges] per CSR slot.
 *   - node tensors are (n, h, d) -> element (v,k,i) at ((v*h + k)*d + i); edge tensors are
 *     (n_edges, h).  h == 1 covers the reference's rank-reduced (n, d) / (n_edges) case.
 *   - outputs are caller-allocated and need NOT be initialised: the callee zero-fills them,
 *     reproducing the reference's at::zeros outputs (graphop_kernel.cu:284,379-380,429,482,
 *     527,571-572): slots no chunk covers read 0.
 *   - `stream` is a hipStream_t (NULL = default stream).  Calls enqueue work and return
 *     without synchronising, like the reference (graphop_kernel.cu:288,302).  No global state;
 *     thread-safe as long as a plan is not destroyed while in use.
 *   - return value: GRAPHOP_OK or an error code; graphop_last_error() gives the message of the
 *     calling thread's last failure (the reference throws c10::Error from AT_ASSERTM /
 *     THCudaCheck instead, graphop.cpp:4-6, graphop_kernel.cu:302).
 *   - `plan` may be NULL.  A plan (graphop_plan_create) caches per-graph derived structure
 *     (row segments, flags, 32-bit index mirrors) for one CSR orientation; with it the kernels
 *     take the row-owned fast paths.  With NULL they take the general path that is correct for
 *     ANY chunk layout (chunks of a row need not be adjacent), merging chunks of a row with
 *     float atomics like the reference's dgl::AtomicAdd (graphop/atomic.cuh:57-96).
 */
#ifndef GRAPHOP_HIP_H_
#define GRAPHOP_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define GRAPHOP_API __attribute__((visibility("default")))
#else
#define GRAPHOP_API
#endif

#define GRAPHOP_ABI_VERSION 8

#define GRAPHOP_F32 0
#define GRAPHOP_F64 1

#define GRAPHOP_OK 0
#define GRAPHOP_ERR_INVALID_ARGUMENT 1 /* bad size / dtype / null pointer / plan mismatch   */
#define GRAPHOP_ERR_HIP 2              /* a HIP runtime call or kernel launch failed        */
#define GRAPHOP_ERR_BAD_GRAPH 3        /* plan validation: index out of range, bad indptr   */

typedef struct graphop_plan graphop_plan_t; /* opaque */

/* Facts about one chunked-CSR orientation, filled by graphop_plan_create. */
typedef struct graphop_plan_info {
  int64_t n_chunks;
  int64_t n_edges;
  int64_t n_segments;      /* maximal runs of adjacent chunks with equal row id              */
  int64_t max_row;         /* largest row id (-1 if no chunks)                               */
  int64_t max_index;       /* largest value in indices (-1 if none / indices == NULL)        */
  int64_t max_segment_len; /* slots in the longest segment                                   */
  int32_t rows_sorted;     /* row[] non-decreasing => a row's chunks are adjacent            */
  int32_t indptr_monotone; /* indptr[] non-decreasing, within [0, n_edges]                   */
  int32_t eid_identity;    /* eid[k] == k for all k                                          */
  int32_t full_coverage;   /* indptr[0] == 0 && indptr[n_chunks] == n_edges                  */
  int32_t row_owned;       /* rows_sorted && indptr_monotone: fast paths enabled             */
  int32_t has_idx32;       /* 32-bit mirrors of eid / indices are cached                     */
  int32_t dense_fill_pct;  /* edges per 32x32 tile of the block-dense cover, in %; 0 = no cover */
  int32_t sorted_in_rows;  /* neighbour ids ascend inside every row segment (window drivers)  */
  int64_t n_dense_blocks;  /* blocks (<= 32 consecutive rows sharing one list of <= 32 ids)   */
  int64_t max_row_gap;     /* ABI 7: longest run of consecutive row ids without a chunk in front of a chunk's row   */
  int64_t n_geometry_fallbacks; /* ABI 7: passes that asked this plan for one window geometry more than it keeps (16) and
                              ran on the chunk drivers instead (2-3x slower on window-friendly shapes; also warned about
                              once per plan on stderr).  Live count: read it with graphop_plan_info after the passes. */
  int32_t sddmm_tile_rows;            /* ABI 8, additive: vrows per tile of the last tile layout analysed for this plan
                                         (csrc/tile_layout.h), 0 = none yet.  Live, like the count above. */
  int32_t sddmm_tile_repeat_permille; /* ... and how many of 1000 slots repeat a neighbour id of their (window, tile) task:
                                         what the tile driver of the SDDMM-type passes does not gather twice */
  int32_t sddmm_tile_max_parts;       /* ... and the largest number of parts (cuts of a task whose slots fit the kernel's LDS
                                         result buffer) any (window, tile) task of that layout has; 0 = none analysed yet, or a
                                         row piece that does not fit the buffer (no layout) */
} graphop_plan_info_t;

GRAPHOP_API int graphop_abi_version(void);
GRAPHOP_API const char* graphop_last_error(void);
/* Device-side failures.  The walk kernels' hand-overs between worker and feeder waves are bounded spins (a launch
 * must not be able to hang the device); a spin whose bound expires does NOT fall through: the wave stores a code and
 * the launch's sequence number in a host-visible record, its workgroup aborts, and the outputs of that launch -- AND
 * of every launch that consumed them -- are invalid.  Launches are asynchronous, so, like a HIP error of a kernel, the
 * failure is seen by whoever looks next.  ABI 7: the record is STICKY -- every compute entry point looks at it first
 * and fails with GRAPHOP_ERR_HIP (message: which pass, on which device, which hand-over) for as long as it is set; only
 * graphop_check_device_errors() reports AND clears it (synchronise the stream first to learn about the launches before
 * it).  A binding should call it where results leave the library (the bundled ones do at the end of every step:
 * functions.attention_step, dist.ShardedAttention.step; bench.py before it prints).  One record per process: with
 * several devices the message names the device of the failed launch. */
GRAPHOP_API int graphop_check_device_errors(void);

/* ---- tuning knobs (also read once from the environment as GRAPHOP_<KEY>) ----------------------
 * keys: sddmm_cpg, spmm_cpg (chunks per lane group of the chunk drivers), force_generic,
 * sweep (0/1: window-owner drivers -- XCDs own column windows and waves pull (window, row tile) tasks),
 * window_kb, mall_window_kb, max_windows, sweep_min_kb, sweep_bpc, sweep_k, vrow_t, sweep_min_granule,
 * sweep_w, spmm_window_scale, staged_ids, dense_blocks (0/1: fp32-MFMA block-dense drivers when the plan found a
 * cover), dense_min_fill, dense_detect_min_fill (percent of a 32x32 tile), attn_fused (0/1),
 * attn_window_scale, attn_k, attn_bpc (fused attention kernels), touch_sddmm (per-task id-line
 * touches of the SDDMM strips), walk (bit 1 row-major SpMM-type, bit 2 column-major SpMM-type passes on
 * the walk drivers: lane groups own rows for a whole round and walk all column windows, nothing is
 * flushed per window), walk_window_kb, walk_window_kb_col, walk_drift, walk_steps, walk_min_bin,
 * walk_blocks, walk_debug, walk_fault (tests: hand-over fault injection), spmm_selfzero, spmm_selfzero_min_mb
 * (row-owning chunk driver defines every output row itself: no zero fill of outputs of at least that many MB),
 * sddmm_tile (SDDMM-type passes, fp32, one head, d = 64, identity eid: 0 window-owner strips, 1 the tile driver -- a
 * workgroup gathers each neighbour row once per (window, tile of sddmm_tile_rows row pieces) -- where at least
 * sddmm_tile_min_repeat percent of the plan's slots repeat a neighbour of their tile, 2 wherever the shape is in scope),
 * sddmm_tile_rows (128, 192, 256, 384), sddmm_tile_min_repeat, sddmm_tile_touch (0/1: L2 touches of the next task's records),
 * plan_trim (0/1: plans drop builder inputs no kernel reads, see "device memory of plans"), spmm_flat (0/1), spmm_flat_max_mean, spmm_flat_min_chunks, spmm_flat_cpg (that driver in its slot-walking form below
 * that many slots per chunk on average, for chunk lists at least that long, with that many chunks per lane group).  Not thread-safe against
 * concurrent op calls; results never depend on them.  (Removed in ABI 6: sweep_mode, sweep_drift,
 * sweep_prefetch, transpose_scalars -- the paced vrow-owner sweep and the scalar transpose pre-pass,
 * both measured slower than what replaced them.) */
GRAPHOP_API int graphop_tune(const char* key, int value);
/* Every knob back to its default (the value at library load: built-in, or GRAPHOP_<KEY> from the
 * environment).  Tests that turn knobs restore them with this, never with literals. */
GRAPHOP_API int graphop_tune_reset(void);
/* Read a knob; enumerate the knob names (i = 0, 1, ...; NULL past the last one). */
GRAPHOP_API int graphop_tune_get(const char* key, int* value);
GRAPHOP_API const char* graphop_tune_key(int i);
/* Device bytes currently held through the library's allocator hook / hipMalloc: plans, their window
 * structures and id layouts, setup temporaries.  What a binding's plan cache budgets against. */
GRAPHOP_API int64_t graphop_memory_bytes(void);
/* ABI 8, additive: floats of the LDS result buffer the tile driver of the SDDMM-type passes has at `rows` vrows per tile --
 * the largest number of slots a part of a (window, tile) task holds (info.sddmm_tile_max_parts counts the parts); 0 where
 * `rows` is not one of sddmm_tile_rows' values.  Not an error code. */
GRAPHOP_API int graphop_sddmm_tile_cap(int rows);

/* ---- device memory of plans ------------------------------------------------------------------
 * Plans own device arrays (per orientation: 8 B per chunk and 4-8 B per edge per dealt / walk layout in use; the 32-bit
 * mirrors of the slot arrays (4-8 B per edge) and a window structure's tables (8 B x windows x rows) are builder inputs:
 * kept only while a per-batch window kernel reads them at run time, otherwise dropped once the layouts exist and
 * rebuilt on demand -- knob plan_trim.  Reddit-shape, both orientations: 2.3 GB once the 8-function step has run,
 * 3.8 GB with the fused op's layouts next to them; round 4: 5.7 GB).
 * By default they come from hipMalloc / hipFree (each a device-wide synchronisation).  A binding
 * may route them through its framework's allocator: alloc_fn(bytes, device, stream) returns a
 * device pointer usable on `stream` (NULL = out of memory), free_fn(ptr) releases it with
 * stream-ordered semantics.  The Python binding registers torch's caching allocator, so plan
 * memory shows up in (and can be reclaimed by) torch.cuda's accounting.  Pass NULL, NULL to
 * restore the default; pointers handed out earlier are still freed through the callback that
 * made them (or left to process exit once it is gone). */
typedef void* (*graphop_alloc_fn)(size_t bytes, int device, void* stream);
typedef void (*graphop_free_fn)(void* ptr);
GRAPHOP_API int graphop_set_allocator(graphop_alloc_fn alloc_fn, graphop_free_fn free_fn);

/* ---- per-kernel timing (measurement aid, off by default) -----------------------------------
 * When enabled, every hot-path kernel launch is bracketed by two hipEvents recorded on the
 * launch stream.  graphop_profile_read synchronises them, aggregates per pass tag
 * ("sddmm_fwd", "softmax_fwd", "spmm_fwd", "spmm_bwd_dedata", "spmm_bwd_dx", "softmax_bwd",
 * "sddmm_bwd_dA", "sddmm_bwd_dB", ...; output zero fills and task-queue resets are recorded under
 * "zero_fill"), clears the log and returns the number of tags. */
typedef struct graphop_profile_rec {
  char name[48];   /* pass tag */
  char kernel[48]; /* device kernel family that executed it (last launch under this tag) */
  int64_t calls;
  double total_ms;
  double min_ms;
  double max_ms;
} graphop_profile_rec_t;
GRAPHOP_API int graphop_profile_enable(int on);
GRAPHOP_API int graphop_profile_read(graphop_profile_rec_t* out, int cap);

/* ---- partition_csr (replaces part_csr.py:13-27 for device-resident indptr) -----------------
 * count: writes per-row chunk counts' exclusive prefix sum to first_chunk[n_rows+1]
 *        (first_chunk[n_rows] = C).  The caller reads C back (one 8-byte D2H copy) to size the
 *        outputs, then calls fill.  scratch: none.
 * fill:  row[C], indptr_out[C+1]. */
GRAPHOP_API int graphop_partition_csr_count(const int64_t* indptr, int64_t n_rows, int64_t chunk_size,
                                int64_t* first_chunk, void* stream);
GRAPHOP_API int graphop_partition_csr_fill(const int64_t* indptr, const int64_t* first_chunk, int64_t n_rows,
                               int64_t chunk_size, int64_t n_chunks, int64_t* row,
                               int64_t* indptr_out, void* stream);

/* ---- plan --------------------------------------------------------------------------------
 * Analyses (row, indptr, eid, indices) on the device, validates it (indices in [0,n_index_bound),
 * eid in [0,n_edges), indptr within range) and caches derived arrays.  Synchronises `stream`
 * once (setup path).  indices may be NULL (softmax / node_mul_edge only need row/indptr/eid).
 * n_index_bound <= 0 skips the range check of indices.  The arrays must stay alive and
 * unmodified while the plan is used.
 * RANGE CHECKS NEED A PLAN: an op entry point compares the plan's largest row id / neighbour id with
 * the operand sizes it is given (too few rows -> GRAPHOP_ERR_INVALID_ARGUMENT, no launch).  Called
 * with plan = NULL (or a plan of other arrays) it has nothing to compare with and keeps the
 * reference's behaviour: ids beyond an operand are out-of-bounds device accesses
 * (graphop_kernel.cu does no shape validation at all).  Bindings that cannot vouch for the ids should
 * always pass a plan; both bundled bindings do. */
GRAPHOP_API int graphop_plan_create(const int64_t* row, const int64_t* indptr, const int64_t* eid,
                        const int64_t* indices, int64_t n_chunks, int64_t n_edges,
                        int64_t n_index_bound, void* stream, graphop_plan_t** plan_out);
GRAPHOP_API int graphop_plan_info(const graphop_plan_t* plan, graphop_plan_info_t* info_out);
GRAPHOP_API void graphop_plan_destroy(graphop_plan_t* plan);

/* Build now every cached structure the ops would otherwise build on first use for node tensors of
 * n_table_rows x (h*d) values gathered through this plan (the column-window structures of the
 * SDDMM-type, SpMM-type and -- fused != 0 -- fused attention passes: fused = 1 for either side,
 * 2 when the plan is only ever the row-major side, 3 the column-major side).  After it no op call on
 * these shapes allocates or synchronises: required before capturing the ops into a HIP graph
 * (an op that would have to build one during capture fails with GRAPHOP_ERR_INVALID_ARGUMENT).
 * Also builds the walk layouts (csrc/kernels_walk.h) of the passes that take them.  Walk layouts are
 * not part of the persistence interface below: a plan re-created by graphop_plan_import rebuilds them
 * on first use (or in graphop_plan_prepare) from the imported arrays, a few milliseconds. */
GRAPHOP_API int graphop_plan_prepare(graphop_plan_t* plan, int dtype, int64_t n_table_rows, int64_t h,
                         int64_t d, int fused, void* stream);

/* ---- plan persistence (graph container) ---------------------------------------
 * A plan's derived arrays can be read out and a plan re-created from them WITHOUT analysing the
 * graph again (graphs.save_graph / load_graph keep them next to the eight index arrays).
 * graphop_plan_array: device pointer and byte size of one array.  sweep < 0: "seg_chunk" (int64
 * [n_segments+1]), "idx32", "eid32" (int32 [n_edges]), "long_segs" (int32), "blk_seg", "seg_e0",
 * "seg_row" (int32; block-dense cover); sweep = i >= 0: "vr_row" (int32 [V]), "wp_lo", "wp_hi"
 * (int32 [W*V]) of the i-th window structure.  Absent arrays give NULL / 0.
 * graphop_plan_import trusts its inputs (they come from an export of the same graph); all
 * pointers are device pointers and are copied. */
typedef struct graphop_sweep_info {
  int64_t win_cols; /* neighbour ids per column window */
  int32_t W;        /* windows */
  int32_t T;        /* row pieces are at most T slots long */
  int32_t V;        /* row pieces ("vrows") */
  int32_t n_dealt;  /* window-major id layouts built on this structure so far (export: see below) */
} graphop_sweep_info_t;
GRAPHOP_API int graphop_plan_n_sweeps(const graphop_plan_t* plan);
GRAPHOP_API int graphop_plan_sweep_info(const graphop_plan_t* plan, int sweep, graphop_sweep_info_t* out);
GRAPHOP_API int graphop_plan_array(const graphop_plan_t* plan, const char* name, int sweep, const void** ptr,
                       int64_t* bytes);
GRAPHOP_API int graphop_plan_import(const int64_t* row, const int64_t* indptr, const int64_t* eid,
                        const int64_t* indices, const graphop_plan_info_t* info,
                        const int64_t* seg_chunk, const int32_t* idx32, const int32_t* eid32,
                        const int32_t* long_segs, int64_t n_long, const int32_t* blk_seg,
                        const int32_t* seg_e0, const int32_t* seg_row, void* stream,
                        graphop_plan_t** plan_out);
GRAPHOP_API int graphop_plan_import_sweep(graphop_plan_t* plan, const graphop_sweep_info_t* info,
                              const int32_t* vr_row, const int32_t* wp_lo, const int32_t* wp_hi,
                              void* stream);
/* The window-owner kernels read their neighbour ids from a window-major copy ("dealt layout": the
 * granules of every task dealt to the lane groups once, each group's ids one contiguous run), one
 * per lane-group geometry (L lanes per group, K row pieces per group).  It is a pure function of
 * the window structure and the 32-bit mirrors, so a container stores only the (L, K) pairs:
 * graphop_plan_sweep_dealt reads the i-th pair of a structure, graphop_plan_sweep_build_dealt
 * re-creates the layout on the (imported) structure that matches `info`. */
GRAPHOP_API int graphop_plan_sweep_dealt(const graphop_plan_t* plan, int sweep, int i, int32_t* L, int32_t* K);
GRAPHOP_API int graphop_plan_sweep_build_dealt(graphop_plan_t* plan, const graphop_sweep_info_t* info, int32_t L,
                                   int32_t K, void* stream);

/* ---- SDDMM: maskedmm_csr_forward(row, indptr, eid, indices, A, B) -> y ----------------------
 * replaces graphop.cpp:16-30 / graphop_kernel.cu:269-304 (kernel :40-55).
 * y[eid[j], k] = <A[row[c], k, :], B[indices[j], k, :]> for every slot j of every chunk c.
 * A: (n_a,h,d)  B: (n_b,h,d)  y: (n_edges,h). */
GRAPHOP_API int graphop_maskedmm_csr_forward(int dtype, const int64_t* row, const int64_t* indptr,
                                 const int64_t* eid, const int64_t* indices, const void* A,
                                 const void* B, void* y, int64_t n_chunks, int64_t n_edges,
                                 int64_t n_a, int64_t n_b, int64_t h, int64_t d,
                                 const graphop_plan_t* plan, void* stream);

/* ---- SDDMM over a SUBSET of the slots into a shared result array (ABI 7; not in the reference) -------------
 * Same arithmetic as graphop_maskedmm_csr_forward -- y[eid[j], k] = <A[row[c], k, :], B[indices[j], k, :]> for every
 * slot j of every chunk c (graphop_kernel.cu:45-52) -- but eid / indices hold n_slots entries of a SUB-GRAPH whose eid
 * values index a result array of n_y >= n_slots entries, and NOTHING is zero-filled: exactly the entries eid[] names
 * are written, each once.  Several chunk lists over disjoint slot sets can therefore compose one SDDMM into one y with
 * no fill and no add (each edge score is written exactly once, graphop_kernel.cu:51).  The sharded step uses it to run
 * the own-column half of its edges while the halo rows of B are still in flight (custom_op_benchmark_amd/dist.py).
 * No plan: graphop_plan_create bounds eid by the slot count; ids are not range-checked (as for any plan-less call). */
GRAPHOP_API int graphop_maskedmm_csr_forward_partial(int dtype, const int64_t* row, const int64_t* indptr,
                                         const int64_t* eid, const int64_t* indices, const void* A,
                                         const void* B, void* y, int64_t n_chunks, int64_t n_slots,
                                         int64_t n_y, int64_t n_a, int64_t n_b, int64_t h, int64_t d,
                                         void* stream);

/* ---- maskedmm_csr_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c,
 *                            A, B, dy) -> [dA, dB]
 * replaces graphop.cpp:108-131 / graphop_kernel.cu:355-409 (kernel :100-112, launched twice).
 * dA[row[c]]  += sum_k dy[eid_r[k]] * B[indices_r[k]]   (row-major CSR)
 * dB[col[c]]  += sum_k dy[eid_c[k]] * A[indices_c[k]]   (column-major CSR)
 * dA may be NULL when n_row_chunks == 0, dB when n_col_chunks == 0 (that half is skipped: the op can
 * be run one orientation at a time). */
GRAPHOP_API int graphop_maskedmm_csr_backward(int dtype, const int64_t* row, const int64_t* indptr_r,
                                  const int64_t* eid_r, const int64_t* indices_r,
                                  const int64_t* col, const int64_t* indptr_c,
                                  const int64_t* eid_c, const int64_t* indices_c, const void* A,
                                  const void* B, const void* dy, void* dA, void* dB,
                                  int64_t n_row_chunks, int64_t n_col_chunks, int64_t n_edges,
                                  int64_t n_a, int64_t n_b, int64_t h, int64_t d,
                                  const graphop_plan_t* plan_r, const graphop_plan_t* plan_c,
                                  void* stream);

/* ---- sparse_softmax_forward(row, indptr, eid, x) -> y ---------------------------------------
 * replaces graphop.cpp:59-69 / graphop_kernel.cu:411-463 (kernels :170-202).
 * Per (row r, head t): m = max(-1e9, max x), y = exp(x-m) / sum exp(x-m) over all slots of all
 * chunks with row[c] == r (the -1e9 floor is the reference's max_val fill, :428).
 * workspace: only used when plan is NULL or not row_owned: 2*workspace_rows*h values of `dtype`,
 * workspace_rows > max(row[]) (the reference sizes it by n_edges, :420,426-427). */
GRAPHOP_API int graphop_sparse_softmax_forward(int dtype, const int64_t* row, const int64_t* indptr,
                                   const int64_t* eid, const void* x, void* y, int64_t n_chunks,
                                   int64_t n_edges, int64_t h, void* workspace,
                                   int64_t workspace_rows, const graphop_plan_t* plan,
                                   void* stream);

/* ---- sparse_softmax_backward(row, indptr, eid, y, dy) -> dx ---------------------------------
 * replaces graphop.cpp:163-175 / graphop_kernel.cu:465-507 (kernels :208-230).
 * g[r,t] = sum dy*y ; dx = dy*y - g*y.  workspace: workspace_rows*h values (general path). */
GRAPHOP_API int graphop_sparse_softmax_backward(int dtype, const int64_t* row, const int64_t* indptr,
                                    const int64_t* eid, const void* y, const void* dy, void* dx,
                                    int64_t n_chunks, int64_t n_edges, int64_t h,
                                    void* workspace, int64_t workspace_rows,
                                    const graphop_plan_t* plan, void* stream);

/* ---- vector_spmm_forward(row, indptr, eid, indices, edata, x) -> y --------------------------
 * replaces graphop.cpp:79-93 / graphop_kernel.cu:509-542 (kernel :118-130).
 * y[row[c], k, :] += sum_j edata[eid[j], k] * x[indices[j], k, :];  y: (n_y,h,d) where the
 * reference uses n_y = n_x (zeros_like(x), :527). */
GRAPHOP_API int graphop_vector_spmm_forward(int dtype, const int64_t* row, const int64_t* indptr,
                                const int64_t* eid, const int64_t* indices, const void* edata,
                                const void* x, void* y, int64_t n_chunks, int64_t n_edges,
                                int64_t n_x, int64_t n_y, int64_t h, int64_t d,
                                const graphop_plan_t* plan, void* stream);

/* ---- vector_spmm_backward(row, indptr, eid, indices, col, indptr_t, eid_t, indices_t,
 *                           edata, dy, x) -> [dedata, dx]   (NB: dy before x)
 * replaces graphop.cpp:190-214 / graphop_kernel.cu:544-600 (kernels :135-163).
 * dedata[eid[j], k] = <dy[row[c], k, :], x[indices[j], k, :]>           (row-major CSR)
 * dx[col[c], k, :] += sum_j edata[eid_t[j], k] * dy[indices_t[j], k, :]  (column-major CSR)
 * Every column chunk is processed (the reference sizes that grid by the ROW chunk count,
 * graphop_kernel.cu:566,588 -- a latent bug when the counts differ).
 * dx may be NULL when n_col_chunks == 0 (that half is skipped: the op can be run one orientation at a time). */
GRAPHOP_API int graphop_vector_spmm_backward(int dtype, const int64_t* row, const int64_t* indptr,
                                 const int64_t* eid, const int64_t* indices, const int64_t* col,
                                 const int64_t* indptr_t, const int64_t* eid_t,
                                 const int64_t* indices_t, const void* edata, const void* dy,
                                 const void* x, void* dedata, void* dx, int64_t n_row_chunks,
                                 int64_t n_col_chunks, int64_t n_edges, int64_t n_x, int64_t n_dy,
                                 int64_t h, int64_t d, const graphop_plan_t* plan_r,
                                 const graphop_plan_t* plan_c, void* stream);

/* ---- two SpMM-type passes over ONE chunked CSR as one launch (ABI 7; not in the reference) ---------------
 *   out0[row[c], :] += sum_j w2[eid[j], 0] * X0[indices[j], :]      out1[row[c], :] += sum_j w2[eid[j], 1] * X1[indices[j], :]
 * -- the arithmetic of two vector_spmm_forward-type kernel launches (graphop_kernel.cu:118-130; in the backward of the
 * composed step: dV = SpMM(a, dO) and dK = SpMM(ds, Q) over the column-major CSR, :151-163 and :100-112) that share
 * their slot list.  w2 is (n_edges, 2): a slot's two weights are ONE 8-byte read, and ids / edge ids / chunk metadata
 * are streamed once.  The sharded step uses it for its column-major side, whose per-slot weights are a random gather
 * (custom_op_benchmark_amd/dist.py).  X0, X1: (n_x, d); out0, out1: (n_out, d), need not be initialised.
 * Supported (graphop_spmm_pair_supported != 0): fp32, one head, d in {64, 128, 256}, a plan of these arrays with sorted
 * rows, 16-byte-aligned outputs; otherwise GRAPHOP_ERR_INVALID_ARGUMENT -- run the two passes separately.
 * Measured on the column side of a papers100M-shape 1/8 shard (tools/pair_columns_experiment.py): 56.9 ms for the two
 * separate launches, 52.4 for this one; writing the pairs in the CSR's slot order first so that the weights stream (built,
 * measured, removed) makes the launch 47.4 ms but the 200 M scattered 8-byte stores cost 8.3. */
/* out2[i] = (w0[i], w1[i]), i < n: two fp32 per-edge arrays interleaved into the (n, 2) pairs graphop_spmm_pair reads
 * (16-byte-aligned arrays; a streaming kernel). */
GRAPHOP_API int graphop_interleave_pairs(int dtype, const void* w0, const void* w1, void* out2, int64_t n, void* stream);
GRAPHOP_API int graphop_spmm_pair_supported(int dtype, int64_t n_chunks, int64_t n_edges, int64_t n_x, int64_t h,
                                int64_t d, const graphop_plan_t* plan);
GRAPHOP_API int graphop_spmm_pair(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                      const int64_t* indices, const void* w2, const void* X0, const void* X1, void* out0,
                      void* out1, int64_t n_chunks, int64_t n_edges, int64_t n_x, int64_t n_out, int64_t h,
                      int64_t d, const graphop_plan_t* plan, void* stream);
/* ---- node_mul_edge_forward(row, indptr, eid, A, B) -> y -------------------------------------
 * replaces graphop.cpp:39-51 / graphop_kernel.cu:235-266 (kernel :19-34).
 * y[eid[j], k] = <A[row[c], k, :], B[eid[j], :]>;  B: (n_edges, d) shared by all heads. */
GRAPHOP_API int graphop_node_mul_edge_forward(int dtype, const int64_t* row, const int64_t* indptr,
                                  const int64_t* eid, const void* A, const void* B, void* y,
                                  int64_t n_chunks, int64_t n_edges, int64_t n_a, int64_t h,
                                  int64_t d, const graphop_plan_t* plan, void* stream);

/* ---- node_mul_edge_backward(row, indptr, eid, A, B, dy) -> [dA, dB] -------------------------
 * replaces graphop.cpp:141-154 / graphop_kernel.cu:306-351 (kernels :61-94).
 * dA[row[c], k, i] += sum_j dy[eid[j], k] * B[eid[j], i];  dB[eid[j], i] = sum_k dy[eid[j],k]*A[row[c],k,i] */
GRAPHOP_API int graphop_node_mul_edge_backward(int dtype, const int64_t* row, const int64_t* indptr,
                                   const int64_t* eid, const void* A, const void* B,
                                   const void* dy, void* dA, void* dB, int64_t n_chunks,
                                   int64_t n_edges, int64_t n_a, int64_t h, int64_t d,
                                   const graphop_plan_t* plan, void* stream);

/* ---- GAT additive attention scores (ABI 8; EXTRA op, not one of the reference's eight) ------------------
 * gat_scores_forward(row, indptr, eid, indices, el, er, negative_slope) -> y
 *   y[eid[j], k] = LeakyReLU(el[row[c], k] + er[indices[j], k]),  LeakyReLU(z) = z > 0 ? z : z * negative_slope
 *   for every slot j of every chunk c (the slot walk of maskedmm_csr_forward); el: (n_l, h), er: (n_r, h) per-node,
 *   per-head scalars, y: (n_edges, h).  One add and at most one multiply per value: bitwise equal to torch's
 *   leaky_relu(el[src] + er[dst]) in the same dtype.
 * gat_scores_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, dy, negative_slope)
 *   -> [del, der], with g[e, k] = dy[e, k] * (z > 0 ? 1 : negative_slope) and z = el[i, k] + er[j, k] recomputed
 *   (the tie z == 0 takes the slope, as torch's leaky_relu_backward):
 *   del[row[c], k] += sum_j g[eid_r[j], k]   (row-major CSR)      der[col[c], k] += sum_j g[eid_c[j], k]   (column-major CSR)
 *   del may be NULL when n_row_chunks == 0, der when n_col_chunks == 0 (that half is skipped).
 * With a plan of the same arrays, fp32 and h in {1, 2, 4, 8, 16} take the fast kernels (csrc/kernels_gat.h); NULL
 * plans, fp64 and other h take the generic ones.  Any chunk layout works on both. */
GRAPHOP_API int graphop_gat_scores_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                               const int64_t* indices, const void* el, const void* er, void* y, int64_t n_chunks,
                               int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, double negative_slope,
                               const graphop_plan_t* plan, void* stream);
GRAPHOP_API int graphop_gat_scores_backward(int dtype, const int64_t* row, const int64_t* indptr_r,
                                const int64_t* eid_r, const int64_t* indices_r, const int64_t* col,
                                const int64_t* indptr_c, const int64_t* eid_c, const int64_t* indices_c,
                                const void* el, const void* er, const void* dy, void* del, void* der,
                                int64_t n_row_chunks, int64_t n_col_chunks, int64_t n_edges, int64_t n_l,
                                int64_t n_r, int64_t h, double negative_slope, const graphop_plan_t* plan_r,
                                const graphop_plan_t* plan_c, void* stream);

/* ---- GATv2 attention scores (ABI 8, additive; EXTRA op, not one of the reference's eight) -------------------------
 * The score of GATv2 (Brody et al.; GATv2Conv in PyG and DGL): the attention vector sits outside the non-linearity.
 * gatv2_scores_forward(row, indptr, eid, indices, xl, xr, att, negative_slope) -> y
 *   y[eid[j], k] = sum_c att[k, c] * LeakyReLU(xl[row[c], k, c] + xr[indices[j], k, c])
 *   for every slot j of every chunk c, LeakyReLU(z) = z > 0 ? z : z * negative_slope;  xl: (n_l, h, d), xr: (n_r, h, d),
 *   att: (h, d), y: (n_edges, h).  Edges that no slot names read 0.  The sum over c runs in the kernel's own order, so y
 *   is NOT bitwise torch's (leaky_relu(xl[src] + xr[dst]) * att).sum(-1): it agrees to rounding.
 * gatv2_scores_backward(row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, att, dy, negative_slope)
 *   -> [dxl, dxr, datt], with z[e, k, c] = xl[i, k, c] + xr[n, k, c] recomputed (nothing E-sized is saved) and
 *   g[e, k, c] = dy[e, k] * att[k, c] * (z > 0 ? 1 : negative_slope)   (the tie z == 0 takes the slope, as torch's
 *   leaky_relu_backward):
 *   dxl[row[c]] += sum_j g[eid_r[j]]   and   datt[k, c] = sum_j dy[eid_r[j], k] * LeakyReLU(z[eid_r[j], k, c])   (row-major CSR)
 *   dxr[col[c]] += sum_j g[eid_c[j]]                                                                            (column-major CSR)
 *   dxl and datt may be NULL when n_row_chunks == 0, dxr when n_col_chunks == 0 (that half is skipped).
 *   workspace: at least min(ceil(n_row_chunks / 16), 8192) * h * d values of `dtype` (per-workgroup partial sums of
 *   datt, added in a fixed order: datt of the fast path is reproducible bit for bit); a smaller one is
 *   GRAPHOP_ERR_INVALID_ARGUMENT; it may be NULL when that is 0.
 * With a plan of the same arrays, fp32, h in {1, 2, 4, 8}, d in {8, 16, 32, 64}, h * d in {64, 128, 256}, ids below
 * 2^31 and 16-byte-aligned tables the fast kernels run (csrc/kernels_gatv2.h); everything else takes the generic ones
 * (one atomic per chunk and element at most).  Any chunk layout works on both. */
GRAPHOP_API int graphop_gatv2_scores_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                 const int64_t* indices, const void* xl, const void* xr, const void* att, void* y,
                                 int64_t n_chunks, int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, int64_t d,
                                 double negative_slope, const graphop_plan_t* plan, void* stream);
GRAPHOP_API int graphop_gatv2_scores_backward(int dtype, const int64_t* row, const int64_t* indptr_r,
                                  const int64_t* eid_r, const int64_t* indices_r, const int64_t* col,
                                  const int64_t* indptr_c, const int64_t* eid_c, const int64_t* indices_c,
                                  const void* xl, const void* xr, const void* att, const void* dy, void* dxl,
                                  void* dxr, void* datt, void* workspace, int64_t workspace_bytes,
                                  int64_t n_row_chunks, int64_t n_col_chunks, int64_t n_edges, int64_t n_l,
                                  int64_t n_r, int64_t h, int64_t d, double negative_slope,
                                  const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream);

/* ---- fused GATv2 attention (ABI 8, additive; EXTRA op, not one of the reference's eight) ---------------------------
 * The layer gatv2_scores_forward -> sparse_softmax_forward -> vector_spmm_forward(a, xr) as one forward and one backward
 * entry, with no E-sized tensor in either direction.  The aggregated table is xr itself (the GATv2Conv convention).  Per
 * head k, for every slot j of every chunk c with i = row[c], n = indices[j]:
 *   z_inc = xl[i, k, c] + xr[n, k, c],  s_in = sum_c att[k, c] * LeakyReLU(z_inc)
 *   m_i = max(-1e9, max_n s_in),  l_i = sum_n exp(s_in - m_i),  a_in = exp(s_in - m_i) / l_i
 *   o[i, k, :] = sum_n a_in xr[n, k, :],  stats[(i*h + k)*2 + {0,1}] = (m_i, 1 / l_i); a row without slots gets o = 0 and
 *   stats (-1e9, 0)
 * gatv2_attention_forward(row, indptr, eid, indices, xl, xr, att, negative_slope) -> [o, stats]
 *   xl (n_l, h, d), xr (n_r, h, d), att (h, d), o (n_l, h, d), stats (n_l, h, 2).
 * gatv2_attention_backward(<8 csr>, xl, xr, att, o, stats, dO, negative_slope) -> [dxl, dxr, datt], z, s and a recomputed
 * per slot:
 *   D_i = <dO_i, o_i>, da_in = <dO_i, xr_n>, ds_in = a_in (da_in - D_i), t_inc = (z_inc > 0 ? 1 : negative_slope) (the tie
 *   z == 0 takes the slope)
 *   dxl[i, k, c] = att[k, c] sum_n ds_in t_inc  and  datt[k, c] = sum_in ds_in LeakyReLU(z_inc)          (row-major CSR)
 *   dxr[n, k, c] = sum_i (ds_in att[k, c] t_inc + a_in dO[i, k, c])                                     (column-major CSR)
 *   dxl and datt may be NULL when n_row_chunks == 0, dxr when n_col_chunks == 0 (that half is skipped).
 *   workspace: at least n_l * h * 4 values of `dtype` (the per-(node, head) items (m, 1 / l, D, 0) the passes read) plus
 *   min(ceil(n_row_chunks / 16), 8192) * h * d values (per-workgroup partial sums of datt, added in a fixed order: datt
 *   of the fast path is reproducible bit for bit); a smaller one is GRAPHOP_ERR_INVALID_ARGUMENT.
 * eid is validated and used for plan lookup only.  With a plan of the same arrays, fp32, h in {1, 2, 4, 8}, d in
 * {8, 16, 32, 64}, h * d in {64, 128, 256}, ids below 2^31 and 16-byte-aligned tables the fast kernels run
 * (csrc/kernels_gatv2_attn.h; the forward needs a row_owned plan: sorted chunk list, monotone indptr; it uses no atomics,
 * so o and stats are reproducible bit for bit); everything else takes the generic ones.  Any chunk layout works on both. */
GRAPHOP_API int graphop_gatv2_attention_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                    const int64_t* indices, const void* xl, const void* xr, const void* att, void* o,
                                    void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_l, int64_t n_r,
                                    int64_t h, int64_t d, double negative_slope, const graphop_plan_t* plan,
                                    void* stream);
GRAPHOP_API int graphop_gatv2_attention_backward(int dtype, const int64_t* row, const int64_t* indptr_r,
                                     const int64_t* eid_r, const int64_t* indices_r, const int64_t* col,
                                     const int64_t* indptr_c, const int64_t* eid_c, const int64_t* indices_c,
                                     const void* xl, const void* xr, const void* att, const void* o, const void* stats,
                                     const void* dO, void* dxl, void* dxr, void* datt, void* workspace,
                                     int64_t workspace_bytes, int64_t n_row_chunks, int64_t n_col_chunks,
                                     int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, int64_t d,
                                     double negative_slope, const graphop_plan_t* plan_r,
                                     const graphop_plan_t* plan_c, void* stream);

/* ---- fused GAT attention (ABI 8, additive; EXTRA op, not one of the reference's eight) -----------------------------
 * The layer gat_scores_forward -> sparse_softmax_forward -> vector_spmm_forward as one forward and one backward entry,
 * with no E-sized tensor in either direction.  Per head k, for every slot j of every chunk c with i = row[c]:
 *   s_ij = LeakyReLU(el[i, k] + er[indices[j], k])      (bitwise what gat_scores_forward computes)
 *   m_i = max(-1e9, max_j s_ij),  l_i = sum_j exp(s_ij - m_i),  o[i, k, :] = sum_j exp(s_ij - m_i) / l_i * V[indices[j], k, :]
 *   stats[(i*h + k)*2 + {0,1}] = (m_i, 1 / l_i)   (n_l, h, 2); a row without slots gets o = 0 and stats (-1e9, 0)
 * gat_attention_forward(row, indptr, eid, indices, el, er, V, negative_slope) -> [o, stats]
 *   el (n_l, h), er (n_r, h), V (n_r, h, d), o (n_l, h, d), stats (n_l, h, 2).
 * gat_attention_backward(<8 csr>, el, er, V, o, stats, dO, negative_slope) -> [del, der, dV], a recomputed per slot:
 *   D_i = <dO_i, o_i>, a_ij = exp(s_ij - m_i) / l_i, ds_ij = a_ij (<dO_i, V_j> - D_i), dz_ij = ds_ij (z > 0 ? 1 : slope)
 *   del[i] = sum_j dz_ij (row-major CSR),  der[j] = sum_i dz_ij,  dV[j] = sum_i a_ij dO_i (column-major CSR).
 *   workspace: at least n_l * h * 4 values of `dtype` (the per-(node, head) items (el, m, 1 / l, D) the passes gather);
 *   a smaller one is GRAPHOP_ERR_INVALID_ARGUMENT.  del may be NULL when n_row_chunks == 0, der and dV when
 *   n_col_chunks == 0.
 * eid is validated and used for plan lookup only.  With a plan of the same arrays, fp32, h in {1, 2, 4, 8}, d in
 * {8, 16, 32, 64}, h * d in {64, 128, 256} and 16-byte-aligned tables the fast kernels run (csrc/kernels_gat_attn.h);
 * everything else takes the generic ones.  Any chunk layout works on both. */
GRAPHOP_API int graphop_gat_attention_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                  const int64_t* indices, const void* el, const void* er, const void* V, void* o,
                                  void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_l, int64_t n_r,
                                  int64_t h, int64_t d, double negative_slope, const graphop_plan_t* plan,
                                  void* stream);
GRAPHOP_API int graphop_gat_attention_backward(int dtype, const int64_t* row, const int64_t* indptr_r,
                                   const int64_t* eid_r, const int64_t* indices_r, const int64_t* col,
                                   const int64_t* indptr_c, const int64_t* eid_c, const int64_t* indices_c,
                                   const void* el, const void* er, const void* V, const void* o, const void* stats,
                                   const void* dO, void* del, void* der, void* dV, void* workspace,
                                   int64_t workspace_bytes, int64_t n_row_chunks, int64_t n_col_chunks,
                                   int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, int64_t d,
                                   double negative_slope, const graphop_plan_t* plan_r,
                                   const graphop_plan_t* plan_c, void* stream);

/* ---- attention dropout for the fused GAT layer (ABI 8, additive; EXTRA ops) ---------------------------------------
 * The fused GAT attention with dropout on the attention weights, attn_drop(edge_softmax(s)), still without any E-sized
 * tensor: the keep decision of edge (i, j) and head k is a pure function of (i, j, k, seed, offset, p), recomputed in
 * each gather pass:
 *   w[0..3] = Philox4x32-10(counter = (i, j, k >> 2, offset), key = (seed & 0xffffffff, seed >> 32))
 *   keep = w[k & 3] >= T with T = floor(p * 2^32);  m_ijk = keep ? 1 / (1 - p) : 0   (both computed in double)
 * i is the row-major row id (index into el / o), j the neighbour id (index into er / V), in both orientations.  The
 * decision does not depend on chunking, plans, orientation or edge numbering; parallel edges (the same (i, j) more
 * than once) share one decision.
 *   forward : o[i] = sum_j a_ij m_ij V[j]; stats are those of the undropped scores (as gat_attention_forward)
 *   backward: D_i = <dO_i, o_i>, da_ij = m_ij <dO_i, V_j>, ds_ij = a_ij (da_ij - D_i), dz as above,
 *             del[i] = sum_j dz_ij, der[j] = sum_i dz_ij, dV[j] = sum_i a_ij m_ij dO_i    (same workspace rule)
 * Arguments as graphop_gat_attention_forward / _backward with (p, seed, offset) after negative_slope:
 *   0 <= p < 1, seed < 2^63, offset a per-layer / per-step counter (one seed serves a whole model), n_l, n_r < 2^32;
 *   anything else is GRAPHOP_ERR_INVALID_ARGUMENT before the device is touched.  p == 0 runs the kernels of
 *   graphop_gat_attention_forward / _backward (bit-identical results).
 * graphop_edge_dropout_mask writes y[eid[slot], k] = m_ijk, (E, h), over the ROW-MAJOR arrays (i = row[c],
 * j = indices[slot]): the mask of the composed path (a * y between sparse_softmax and vector_spmm) and of tests.
 * Edges that no slot names get 0. */
GRAPHOP_API int graphop_gat_attention_dropout_forward(int dtype, const int64_t* row, const int64_t* indptr,
                                  const int64_t* eid, const int64_t* indices, const void* el, const void* er,
                                  const void* V, void* o, void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_l,
                                  int64_t n_r, int64_t h, int64_t d, double negative_slope, double p, uint64_t seed,
                                  uint32_t offset, const graphop_plan_t* plan, void* stream);
GRAPHOP_API int graphop_gat_attention_dropout_backward(int dtype, const int64_t* row, const int64_t* indptr_r,
                                   const int64_t* eid_r, const int64_t* indices_r, const int64_t* col,
                                   const int64_t* indptr_c, const int64_t* eid_c, const int64_t* indices_c,
                                   const void* el, const void* er, const void* V, const void* o, const void* stats,
                                   const void* dO, void* del, void* der, void* dV, void* workspace,
                                   int64_t workspace_bytes, int64_t n_row_chunks, int64_t n_col_chunks,
                                   int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, int64_t d,
                                   double negative_slope, double p, uint64_t seed, uint32_t offset,
                                   const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream);
GRAPHOP_API int graphop_edge_dropout_mask(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                  const int64_t* indices, void* y, int64_t n_chunks, int64_t n_edges, int64_t n_l,
                                  int64_t n_r, int64_t h, double p, uint64_t seed, uint32_t offset,
                                  const graphop_plan_t* plan, void* stream);

/* ---- attention dropout for the fused GATv2 layer (ABI 8, additive; EXTRA ops) -------------------------------------
 * The fused GATv2 attention with dropout on the attention weights, attn_drop(edge_softmax(s)), still without any
 * E-sized tensor.  The keep decision and the multiplier m_ijk are exactly those of the block above (Philox4x32-10 over
 * (i, j, k >> 2, offset) keyed by the seed, T = floor(p * 2^32), 1 / (1 - p), both computed in double): i is the
 * row-major row id (index into xl / o), j the neighbour id (index into xr), in that order in both orientations;
 * parallel edges share one decision; graphop_edge_dropout_mask writes the same values out as an (E, h) tensor.
 *   forward : o[i, k, :] = sum_n a_in m_in xr[n, k, :]; stats are those of the undropped scores, bit for bit what
 *             graphop_gatv2_attention_forward leaves (the same expressions in the same order)
 *   backward: D_i = <dO_i, o_i>, da_in = m_in <dO_i, xr_n>, ds_in = a_in (da_in - D_i), t_inc as above,
 *             dxl[i, k, c] = att[k, c] sum_n ds_in t_inc,  datt[k, c] = sum_in ds_in LeakyReLU(z_inc),
 *             dxr[n, k, c] = sum_i (ds_in att[k, c] t_inc + a_in m_in dO[i, k, c])               (same workspace rule)
 *   A row whose slots are all dropped for a head has o = 0, D = 0 and dxl = 0 there and adds nothing to dxr or datt.
 * Arguments as graphop_gatv2_attention_forward / _backward with (p, seed, offset) after negative_slope:
 *   0 <= p < 1, seed < 2^63, offset a per-layer / per-step counter (one seed serves a whole model), n_l, n_r < 2^32;
 *   anything else is GRAPHOP_ERR_INVALID_ARGUMENT before the device is touched.  p == 0 runs the kernels of
 *   graphop_gatv2_attention_forward / _backward (bit-identical results, the same profile tags).
 * Fast and generic kernels are chosen as without dropout (csrc/kernels_gatv2_attn.h: k_gv2drop_*_f32 and the
 * DROP = true generic ones); the fast forward still uses no atomics, so o and stats stay reproducible bit for bit. */
GRAPHOP_API int graphop_gatv2_attention_dropout_forward(int dtype, const int64_t* row, const int64_t* indptr,
                                    const int64_t* eid, const int64_t* indices, const void* xl, const void* xr,
                                    const void* att, void* o, void* stats, int64_t n_chunks, int64_t n_edges,
                                    int64_t n_l, int64_t n_r, int64_t h, int64_t d, double negative_slope, double p,
                                    uint64_t seed, uint32_t offset, const graphop_plan_t* plan, void* stream);
GRAPHOP_API int graphop_gatv2_attention_dropout_backward(int dtype, const int64_t* row, const int64_t* indptr_r,
                                     const int64_t* eid_r, const int64_t* indices_r, const int64_t* col,
                                     const int64_t* indptr_c, const int64_t* eid_c, const int64_t* indices_c,
                                     const void* xl, const void* xr, const void* att, const void* o, const void* stats,
                                     const void* dO, void* dxl, void* dxr, void* datt, void* workspace,
                                     int64_t workspace_bytes, int64_t n_row_chunks, int64_t n_col_chunks,
                                     int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, int64_t d,
                                     double negative_slope, double p, uint64_t seed, uint32_t offset,
                                     const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream);

/* ---- fused GAT attention with an edge term (ABI 8, additive; EXTRA ops) ------------------------------------------
 * The fused GAT layer for GATConv(edge_dim=...) / EGATConv, and for a fixed per-edge bias such as log edge weights: per
 * head k, for every slot of every chunk c with i = row[c], j = indices[slot], e = eid[slot],
 *   z_e = (el[i, k] + er[j, k]) + ee[e, k]   (added in that order),   s_e = LeakyReLU(z_e)
 *   m_i = max(-1e9, max s),  l_i = sum exp(s - m_i),  a_e = exp(s_e - m_i) / l_i,  o[i, k, :] = sum a_e m_ijk V[j, k, :]
 *   stats = (m_i, 1 / l_i) of the undropped scores, (n_l, h, 2); a row without slots gets o = 0 and stats (-1e9, 0)
 * m_ijk is the dropout multiplier of graphop_edge_dropout_mask (a function of (i, j, k, seed, offset, p): parallel edges
 * share a decision); p == 0 means no dropout and runs the kernels without the decision.
 * gat_edge_attention_forward(row, indptr, eid, indices, el, er, ee, V, negative_slope, p, seed, offset) -> [o, stats]
 *   el (n_l, h), er (n_r, h), ee (n_edges, h) indexed by EDGE ID, V (n_r, h, d), o (n_l, h, d), stats (n_l, h, 2).
 * gat_edge_attention_backward(<8 csr>, el, er, ee, V, o, stats, dO, ...) -> [del, der, dee, dV], a recomputed per slot:
 *   D_i = <dO_i, o_i>, da_e = m_ijk <dO_i, V_j>, ds_e = a_e (da_e - D_i), dz_e = ds_e (z_e > 0 ? 1 : slope)
 *   del[i] = sum_j dz_e and dee[e, k] = dz_e (row-major CSR),  der[j] = sum_i dz_e,  dV[j] = sum_i a_e m_ijk dO_i
 *   (column-major CSR).  dee (n_edges, h) is the only edge-sized tensor written, one plain store per slot and head;
 *   edge ids that no row-major slot names get 0 (dee is zero-filled unless plan_r proves that every id is written).
 *   dee may be NULL: then nothing edge-sized is written.  del may be NULL when n_row_chunks == 0, der and dV when
 *   n_col_chunks == 0.  workspace: at least n_l * h * 4 values of `dtype`, as for graphop_gat_attention_backward.
 * 0 <= p < 1, seed < 2^63, n_l, n_r < 2^32; anything else is GRAPHOP_ERR_INVALID_ARGUMENT before the device is touched.
 * The fast kernels run under the conditions of graphop_gat_attention_forward plus ee and dee aligned to their item
 * width, 4 * min(h, 4) bytes (csrc/kernels_gat_edge_attn.h); everything else takes the generic ones.  Any chunk layout
 * works on both.  With a row-major plan whose eid is the identity the row-major passes do not read eid. */
GRAPHOP_API int graphop_gat_edge_attention_forward(int dtype, const int64_t* row, const int64_t* indptr,
                                   const int64_t* eid, const int64_t* indices, const void* el, const void* er,
                                   const void* ee, const void* V, void* o, void* stats, int64_t n_chunks,
                                   int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, int64_t d,
                                   double negative_slope, double p, uint64_t seed, uint32_t offset,
                                   const graphop_plan_t* plan, void* stream);
GRAPHOP_API int graphop_gat_edge_attention_backward(int dtype, const int64_t* row, const int64_t* indptr_r,
                                    const int64_t* eid_r, const int64_t* indices_r, const int64_t* col,
                                    const int64_t* indptr_c, const int64_t* eid_c, const int64_t* indices_c,
                                    const void* el, const void* er, const void* ee, const void* V, const void* o,
                                    const void* stats, const void* dO, void* del, void* der, void* dee, void* dV,
                                    void* workspace, int64_t workspace_bytes, int64_t n_row_chunks,
                                    int64_t n_col_chunks, int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h,
                                    int64_t d, double negative_slope, double p, uint64_t seed, uint32_t offset,
                                    const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream);

/* ---- fused GATv2 attention with edge features (ABI 8, additive; EXTRA ops) -----------------------------------------
 * The fused GATv2 layer for GATv2Conv(edge_dim=...): per head k, for every slot of every chunk c with i = row[c],
 * j = indices[slot], e = eid[slot],
 *   z_ec = (xl[i, k, c] + xr[j, k, c]) + xe[e, k, c]   (added in that order),   s_e = sum_c att[k, c] LeakyReLU(z_ec)
 *   m_i = max(-1e9, max s),  l_i = sum exp(s - m_i),  a_e = exp(s_e - m_i) / l_i,  o[i, k, :] = sum a_e m_ijk xr[j, k, :]
 *   stats = (m_i, 1 / l_i) of the undropped scores, (n_l, h, 2); a row without slots gets o = 0 and stats (-1e9, 0)
 * m_ijk is the dropout multiplier of graphop_edge_dropout_mask (a function of (i, j, k, seed, offset, p): parallel edges
 * share a decision but each has its own xe row); p == 0 means no dropout and runs the kernels without the decision.
 * gatv2_edge_attention_forward(row, indptr, eid, indices, xl, xr, xe, att, ...) -> [o, stats]
 *   xl (n_l, h, d), xr (n_r, h, d), xe (n_edges, h, d) indexed by EDGE ID, att (h, d), o (n_l, h, d), stats (n_l, h, 2).
 * gatv2_edge_attention_backward(<8 csr>, xl, xr, xe, att, o, stats, dO, ...) -> [dxl, dxr, dxe, datt], recomputed per slot:
 *   D_i = <dO_i, o_i>, da_e = m_ijk <dO_i, xr_j>, ds_e = a_e (da_e - D_i), t_ec = (z_ec > 0 ? 1 : slope)
 *   dxl[i, k, c] = att[k, c] sum_j ds_e t_ec,  datt[k, c] = sum_e ds_e LeakyReLU(z_ec),  dxe[e, k, c] = ds_e att[k, c] t_ec
 *   (row-major CSR),  dxr[j, k, c] = sum_i (ds_e att[k, c] t_ec + a_e m_ijk dO[i, k, c])  (column-major CSR).
 *   dxe (n_edges, h, d) is the only edge-sized tensor written, one plain store per slot and element; edge ids that no
 *   row-major slot names get 0 (dxe is zero-filled unless plan_r proves that every id is written).  dxe may be NULL:
 *   then nothing edge-sized is written.  dxl and datt may be NULL when n_row_chunks == 0, dxr when n_col_chunks == 0.
 *   workspace: as for graphop_gatv2_attention_backward.
 * 0 <= p < 1, seed < 2^63, n_l, n_r < 2^32; anything else is GRAPHOP_ERR_INVALID_ARGUMENT before the device is touched.
 * The fast kernels run under the conditions of graphop_gatv2_attention_forward plus xe and dxe aligned to 16 bytes
 * (csrc/kernels_gatv2_edge_attn.h); everything else takes the generic ones.  Any chunk layout works on both.  With a
 * row-major plan whose eid is the identity the row-major passes do not read eid. */
GRAPHOP_API int graphop_gatv2_edge_attention_forward(int dtype, const int64_t* row, const int64_t* indptr,
                                     const int64_t* eid, const int64_t* indices, const void* xl, const void* xr,
                                     const void* xe, const void* att, void* o, void* stats, int64_t n_chunks,
                                     int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, int64_t d,
                                     double negative_slope, double p, uint64_t seed, uint32_t offset,
                                     const graphop_plan_t* plan, void* stream);
GRAPHOP_API int graphop_gatv2_edge_attention_backward(int dtype, const int64_t* row, const int64_t* indptr_r,
                                      const int64_t* eid_r, const int64_t* indices_r, const int64_t* col,
                                      const int64_t* indptr_c, const int64_t* eid_c, const int64_t* indices_c,
                                      const void* xl, const void* xr, const void* xe, const void* att, const void* o,
                                      const void* stats, const void* dO, void* dxl, void* dxr, void* dxe, void* datt,
                                      void* workspace, int64_t workspace_bytes, int64_t n_row_chunks,
                                      int64_t n_col_chunks, int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h,
                                      int64_t d, double negative_slope, double p, uint64_t seed, uint32_t offset,
                                      const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream);

/* ---- fused attention step (EXTRA op, not one of the reference's eight) --------------------------
 * The composition the reference harness chains by hand -- MaskedMMCSR -> SparseSoftmax -> VectorSPMM
 * (wrapper.py:20-30, 8-18, 44-55) -- as one forward and one backward entry, so that the E-sized
 * intermediates s, a, da, ds never leave the library:
 *   forward : o[r]  = sum_j a[r,j] V[j],  a = row-softmax(<Q[r], K[j]>) over the row-major CSR;
 *             stats[(r*h + k)*2 + {0,1}] = (row max m, 1 / sum exp(s - m))   (n_q, h, 2)
 *   backward: dQ, dK, dV for a given dO, from (Q, K, V, o, stats): a and ds are recomputed per slot
 *             (a = exp(s - m) / sum, ds = a (<dO_r, V_j> - <dO_r, o_r>)).
 * Results equal the composition of the unfused entry points up to fp32 summation order.
 * Round 4: where it applies (fp32, h == 1, d == 64, a walkable row-major plan with identity eid) the forward is ONE
 * kernel -- a walk-style pass with an online softmax (csrc/kernels_attn_walk.h) -- and s / a are never materialised.
 * workspace: device scratch of graphop_attention_workspace_bytes(...) bytes (forward: piece records of the rows the
 * walk's bins share, a few MB, for the one-pass form; s and a for the composed form;
 * backward: packed operand tables when the fused passes apply -- fp32, h == 1, both plans given;
 * window-owner drivers for sweepable plans and tables beyond the L2, chunk drivers otherwise --
 * else s, a, da, ds of the composed path). */
GRAPHOP_API int graphop_attention_workspace_bytes(int dtype, int backward, int64_t n_edges, int64_t n_q,
                                      int64_t n_k, int64_t h, int64_t d,
                                      const graphop_plan_t* plan_r, const graphop_plan_t* plan_c,
                                      void* stream, int64_t* bytes_out);
/* 1 when graphop_attention_backward will run its fused passes (window-owner or chunk-driver form) for
 * these shapes / plans, 0 when
 * it will compose the unfused entry points (and recompute s and a first): a caller that can keep a
 * from its forward (the Python autograd class does) then prefers the unfused backward ops. */
GRAPHOP_API int graphop_attention_backward_is_fused(int dtype, int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h,
                                        int64_t d, const graphop_plan_t* plan_r,
                                        const graphop_plan_t* plan_c, void* stream, int* fused_out);
GRAPHOP_API int graphop_attention_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                              const int64_t* indices, const void* Q, const void* K, const void* V,
                              void* o, void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_q,
                              int64_t n_k, int64_t h, int64_t d, void* workspace,
                              int64_t workspace_bytes, const graphop_plan_t* plan, void* stream);
GRAPHOP_API int graphop_attention_backward(int dtype, const int64_t* row, const int64_t* indptr_r,
                               const int64_t* eid_r, const int64_t* indices_r, const int64_t* col,
                               const int64_t* indptr_c, const int64_t* eid_c, const int64_t* indices_c,
                               const void* Q, const void* K, const void* V, const void* o,
                               const void* stats, const void* dO, void* dQ, void* dK, void* dV,
                               int64_t n_row_chunks, int64_t n_col_chunks, int64_t n_edges,
                               int64_t n_q, int64_t n_k, int64_t h, int64_t d, void* workspace,
                               int64_t workspace_bytes, const graphop_plan_t* plan_r,
                               const graphop_plan_t* plan_c, void* stream);

/* ---- attention dropout for the fused attention step (ABI 8, additive; EXTRA ops) ------------------------------------
 * The fused step with dropout on the attention weights, attn_drop(softmax(Q K^T)) (TransformerConv(dropout=...),
 * DotGatConv), still without any E-sized mask.  For edge (i, j) -- i indexes Q / o, j indexes K / V -- and GLOBAL head k
 * the multiplier is that of the fused GAT layer, unchanged: m_ijk = keep ? 1 / (1 - p) : 0 with keep from
 * Philox4x32-10 on the counter (i, j, k >> 2, offset) and the key seed (graphop_edge_dropout_mask writes the same values
 * out).  Parallel edges share one decision.
 *   forward : o[i] = sum_j a_ij m_ij V[j]; stats are those of the undropped scores (as graphop_attention_forward)
 *   backward: D_i = <dO_i, o_i>, da_ij = m_ij <dO_i, V_j>, ds_ij = a_ij (da_ij - D_i);
 *             dQ_i = sum_j ds_ij K_j, dK_j = sum_i ds_ij Q_i, dV_j = sum_i a_ij m_ij dO_i
 * A row whose edges are all dropped has o = 0 and dQ = 0 and adds nothing to dK or dV.
 * Arguments as graphop_attention_forward / _backward, then (p, seed, offset, head0) after the stream:
 *   0 <= p < 1, seed < 2^63, n_q and n_k < 2^32 (GRAPHOP_ERR_ARG otherwise).  head0 is the global index of the call's
 *   first head: local head k decides as global head head0 + k, so a caller that hands over one group of heads at a time
 *   makes the decisions of one call over all heads.  p == 0 runs the kernels of graphop_attention_forward / _backward
 *   (bit-identical results).  There is no 1 / sqrt(d) scale argument: fold it into Q.
 * The fused forms (one-pass forward, window-owner and chunk-driver backward) are chosen by the rules of the undropped
 * op and recompute the decision per slot; everything else composes the unfused entry points and multiplies a (and the
 * gradient that comes back) by m in the workspace.  workspace: graphop_attention_dropout_workspace_bytes(...) bytes --
 * the composed backward holds one E-sized array more (a * m) than graphop_attention_workspace_bytes reports. */
GRAPHOP_API int graphop_attention_dropout_workspace_bytes(int dtype, int backward, int64_t n_edges, int64_t n_q,
                                              int64_t n_k, int64_t h, int64_t d, const graphop_plan_t* plan_r,
                                              const graphop_plan_t* plan_c, void* stream, int64_t* bytes_out);
GRAPHOP_API int graphop_attention_dropout_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                      const int64_t* indices, const void* Q, const void* K, const void* V, void* o,
                                      void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_q, int64_t n_k,
                                      int64_t h, int64_t d, void* workspace, int64_t workspace_bytes,
                                      const graphop_plan_t* plan, void* stream, double p, uint64_t seed,
                                      uint32_t offset, int64_t head0);
GRAPHOP_API int graphop_attention_dropout_backward(int dtype, const int64_t* row, const int64_t* indptr_r,
                                       const int64_t* eid_r, const int64_t* indices_r, const int64_t* col,
                                       const int64_t* indptr_c, const int64_t* eid_c, const int64_t* indices_c,
                                       const void* Q, const void* K, const void* V, const void* o,
                                       const void* stats, const void* dO, void* dQ, void* dK, void* dV,
                                       int64_t n_row_chunks, int64_t n_col_chunks, int64_t n_edges, int64_t n_q,
                                       int64_t n_k, int64_t h, int64_t d, void* workspace, int64_t workspace_bytes,
                                       const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream,
                                       double p, uint64_t seed, uint32_t offset, int64_t head0);

/* ---- per-edge score bias for the fused attention step (ABI 8, additive; EXTRA ops) ----------------------------------
 * The fused step with a term per edge inside the softmax (Graphormer-type spatial / edge encodings, relative positional
 * biases, weighted graphs with b = log w, the key-side edge term <Q_i, We x_e> of TransformerConv(edge_dim=...), which
 * graphop_node_mul_edge_forward produces).  For edge e = (i, j) -- i indexes Q / o, j indexes K / V -- and head k, with b
 * indexed by EDGE ID ((n_edges, h), the dtype of Q, contiguous):
 *   s_e  = <Q_i, K_j> + b[e, k]                 (one add, after the dot product's reduction)
 *   a_e  = exp(s_e - m_i) * linv_i              m_i = max(-1e9, row max of s), linv_i = 1 / sum exp(s - m_i)
 *   o_i  = sum_e a_e m_e V_j                    m_e: the multiplier of graphop_attention_dropout_* (1 at p == 0)
 *   ds_e = a_e (m_e <dO_i, V_j> - D_i), D_i = <dO_i, o_i>;  db[e, k] = ds_e;  dQ, dK, dV from ds_e and a_e m_e as without b
 * stats are those of the biased, undropped scores.  b must be FINITE: a bias at or below the -1e9 floor of the row
 * maximum is not a mask (a row whose scores all lie below the floor does not normalise).  No 1 / sqrt(d) argument.
 * Arguments as graphop_attention_dropout_forward / _backward with b after V and, in the backward, db after dV.
 * db == NULL: the gradient of b is not wanted; nothing edge-sized is then written and no kernel stores it.  Otherwise
 * db[e] is written for every edge id a row-major slot names (each once; the others are left untouched).  The checks of
 * the undropped op run first, then those of the dropout arguments, then b != NULL (unless n_edges * h == 0).  p == 0
 * takes no Philox path; empty problems are no-ops that dereference nothing.
 * Forms: where graphop_attention_backward would run either fused form (and GRAPHOP_ATTN_ROWS is not 0) the backward is
 * the chunk-driver form with the bias (k_attn_bias_bwd_rows_f32: b and db addressed through the plans' edge ids); the
 * forward is one chunk-driver pass (k_attn_bias_fwd_rows_f32) for fp32, h == 1, d a power of two in 16..1024 and a
 * matching plan with sorted rows.  Everything else composes the unfused entry points: s += b after the SDDMM, and the
 * softmax backward writes ds into db.
 * Several heads (this op, graphop_attention_* and graphop_attention_dropout_*): fp32 calls whose (h, d) is one of
 * (2,32) (2,64) (4,16) (4,32) (4,64) (8,8) (8,16) (8,32), with matching plans that carry neighbour ids and id ranges
 * inside the tables, run chunk-driver passes over all heads of a row at once (k_attn_heads_fwd_rows_f32 -- the
 * forward also wants sorted rows -- and k_attn_heads_bwd_rows_f32): b and db are then the only edge-sized arrays of the
 * whole call.  Knob attn_heads (GRAPHOP_ATTN_HEADS): -1 by a cost rule (default), 0 never, 1 wherever these
 * conditions hold; GRAPHOP_ATTN_ROWS = 0 forbids this form too.  graphop_attention_backward_is_fused answers 1 for
 * such a call and the three workspace queries report what it needs.
 * workspace: graphop_attention_bias_workspace_bytes(..., with_db, ...) bytes;
 * with_db != 0 names a backward call with db given, whose composed form holds one E-sized array fewer. */
GRAPHOP_API int graphop_attention_bias_workspace_bytes(int dtype, int backward, int64_t n_edges, int64_t n_q, int64_t n_k,
                                           int64_t h, int64_t d, const graphop_plan_t* plan_r,
                                           const graphop_plan_t* plan_c, void* stream, int with_db, int64_t* bytes_out);
GRAPHOP_API int graphop_attention_bias_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                   const int64_t* indices, const void* Q, const void* K, const void* V, const void* b,
                                   void* o, void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_q, int64_t n_k,
                                   int64_t h, int64_t d, void* workspace, int64_t workspace_bytes,
                                   const graphop_plan_t* plan, void* stream, double p, uint64_t seed, uint32_t offset,
                                   int64_t head0);
GRAPHOP_API int graphop_attention_bias_backward(int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                    const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                    const int64_t* eid_c, const int64_t* indices_c, const void* Q, const void* K,
                                    const void* V, const void* b, const void* o, const void* stats, const void* dO,
                                    void* dQ, void* dK, void* dV, void* db, int64_t n_row_chunks, int64_t n_col_chunks,
                                    int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h, int64_t d, void* workspace,
                                    int64_t workspace_bytes, const graphop_plan_t* plan_r, const graphop_plan_t* plan_c,
                                    void* stream, double p, uint64_t seed, uint32_t offset, int64_t head0);

/* ---- edge features in the fused attention step: K_j + xe[e], V_j + xe[e] (ABI 8, additive; EXTRA ops) --------------
 * The fused step with a feature row per edge added to the key AND the value (TransformerConv(edge_dim=...):
 * out = alpha * (value_j + edge_attr); the Dwivedi-Bresson and GraphGPS edge-featured graph transformers).  For edge
 * e = (i, j) -- i indexes Q / o, j indexes K / V -- and head k, with xe indexed by EDGE ID ((n_edges, h, d), the dtype
 * of Q / K / V, contiguous):
 *   kx_e = K_j + xe[e]        vx_e = V_j + xe[e]
 *   s_e  = <Q_i, kx_e>        m_i = max(-1e9, row max of s)   linv_i = 1 / sum_e exp(s_e - m_i)   a_e = exp(s_e - m_i) linv_i
 *   o_i  = sum_e a_e mult_e vx_e           mult_e: the multiplier of graphop_attention_dropout_* for (i, j, head0 + k), 1 at p == 0
 *   D_i  = <dO_i, o_i>        da_e = mult_e <dO_i, vx_e>      ds_e = a_e (da_e - D_i)
 *   dQ_i = sum_e ds_e kx_e    dK_j = sum_e ds_e Q_i           dV_j = sum_e a_e mult_e dO_i
 *   dxe[e] = ds_e Q_i + a_e mult_e dO_i
 * stats (n_q, h, 2) = (m_i, linv_i) of the undropped scores; rows without edges get o = 0 and stats = (-1e9, 0).
 * Parallel edges share a dropout decision and have each their own xe row.  No 1 / sqrt(d) argument (fold it into Q), no
 * bias argument.  Arguments as graphop_attention_bias_forward / _backward with xe where b is and dxe where db is.
 * dxe is the only edge-sized array made.  dxe == NULL: the gradient of xe is not wanted; nothing edge-sized is then
 * written and no kernel stores it.  Otherwise dxe[e] is written for every edge id a row-major slot names (each once; the
 * others are left untouched: zero-fill dxe first where the chunk list may leave slots out).  The checks of
 * graphop_attention_forward run first, then those of the dropout arguments (head0 included), then xe != NULL (unless
 * n_edges * h * d == 0), then the workspace.  p == 0 takes no Philox path; empty problems are no-ops that dereference
 * nothing.  A plan must bound the ids by n_q and n_k (an error otherwise).
 * Forms: fp32 calls whose (h, d) is one of (1,64) (2,32) (2,64) (4,16) (4,32) (4,64) (8,8) (8,16) (8,32), with 16-byte
 * aligned operands and ids below 2^31, run the chunk-driver passes of the several-head kernels with the edge row streamed
 * per slot (kernels_attn_edge.h): the forward (k_attn_edge_fwd_rows_f32) with a matching plan with sorted rows and
 * neighbour ids, each backward pass (k_attn_edge_bwd_rows_f32) with a matching plan of its orientation.  Everything else
 * (fp64, other shapes, no plan, shuffled chunks in the forward, misaligned xe / dxe, GRAPHOP_FORCE_GENERIC) runs the
 * generic kernels k_attn_edge_*_generic, one wave per chunk: the op works for every valid call and never composes.
 * workspace: graphop_attention_edge_workspace_bytes bytes (forward: the piece records of rows that lane groups share;
 * backward: the packed operand tables and the per-(row, head) statistics). */
GRAPHOP_API int graphop_attention_edge_workspace_bytes(int dtype, int backward, int64_t n_edges, int64_t n_q, int64_t n_k,
                                           int64_t h, int64_t d, const graphop_plan_t* plan_r,
                                           const graphop_plan_t* plan_c, void* stream, int64_t* bytes_out);
GRAPHOP_API int graphop_attention_edge_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                   const int64_t* indices, const void* Q, const void* K, const void* V, const void* xe,
                                   void* o, void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_q, int64_t n_k,
                                   int64_t h, int64_t d, void* workspace, int64_t workspace_bytes,
                                   const graphop_plan_t* plan, void* stream, double p, uint64_t seed, uint32_t offset,
                                   int64_t head0);
GRAPHOP_API int graphop_attention_edge_backward(int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                    const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                    const int64_t* eid_c, const int64_t* indices_c, const void* Q, const void* K,
                                    const void* V, const void* xe, const void* o, const void* stats, const void* dO,
                                    void* dQ, void* dK, void* dV, void* dxe, int64_t n_row_chunks, int64_t n_col_chunks,
                                    int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h, int64_t d, void* workspace,
                                    int64_t workspace_bytes, const graphop_plan_t* plan_r, const graphop_plan_t* plan_c,
                                    void* stream, double p, uint64_t seed, uint32_t offset, int64_t head0);

/* ---- edge-type embeddings in the fused attention step: K_j + R[t_e], V_j + R[t_e] (ABI 8, additive; EXTRA ops) ------
 * The step of graphop_attention_edge_* for a CATEGORICAL edge feature (a bond type, a relation of a knowledge graph, a
 * clipped relative position, a hop distance; relation-aware attention, Shaw-type relative positions,
 * TransformerConv(edge_dim=...) behind an nn.Embedding): edge e carries the type t_e = etype[e] and the table row
 * R[t_e] is added to its key AND its value.  etype is (n_edges) int32, contiguous, indexed by EDGE ID, with values in
 * [0, n_types); R is (n_types, h, d) in the dtype of Q / K / V, contiguous.  DESIGN.md 4.5o.
 *   kx_e = K_j + R[t_e]       vx_e = V_j + R[t_e]
 *   every other line of graphop_attention_edge_* with xe[e] := R[t_e]
 *   dR[t] = sum over the edges e with t_e = t of (ds_e Q_i + a_e mult_e dO_i);  types no edge carries get dR[t] = 0
 * Nothing edge-sized is made in either direction: etype is the only edge-sized operand.  Parallel edges share a dropout
 * decision and may differ in type.  No 1 / sqrt(d) argument, no bias argument, no xe together with R.
 * OUT-OF-RANGE TYPES: etype is NOT scanned (a scan would synchronise the stream and break its capture in a graph).
 * Every kernel clamps the type it loads into [0, n_types - 1], as an unsigned value, before it forms an address: a type
 * outside [0, n_types) gives an undefined value (that of some type of the table) and never touches memory outside R / dR.
 * Arguments as graphop_attention_edge_* with (R, etype) where xe is, dR where dxe is and n_types after d.  dR == NULL:
 * the gradient of R is not wanted; nothing is accumulated for it.  Otherwise the call itself writes every element of dR
 * (as it zero-fills dQ, dK, dV and what it accumulates into, with stream-ordered fills: a step can be captured).
 * Checks, all before anything touches a device: those of graphop_attention_forward, then the dropout arguments (head0
 * included), then n_types >= 1 (unless n_edges == 0), then R != NULL and etype != NULL (unless n_edges * h * d == 0),
 * then the workspace.  Empty problems fill what they must and dereference nothing.  A matching plan must bound the ids by
 * n_q and n_k (an error otherwise).
 * Forms, chosen pass by pass: fp32 calls whose (h, d) is one of (1,64) (2,32) (2,64) (4,16) (4,32) (4,64) (8,8) (8,16)
 * (8,32), with 16-byte aligned operands and ids below 2^31, run the chunk-driver passes of graphop_attention_edge_* with
 * the edge piece read from the table (k_attn_etype_fwd_rows_f32, k_attn_etype_bwd_rows_f32) under the same conditions on
 * the plans.  The row pass with dR != NULL sums dR in 4 n_types h d bytes of LDS and so needs that to be at most 16 KiB
 * (n_types <= 4096 / (h d): 64 types at h d = 64, 16 at h d = 256); beyond it that pass alone is the generic one.
 * Everything else runs the generic kernels k_attn_etype_*_generic, one wave per chunk.
 * workspace: graphop_attention_etype_workspace_bytes bytes.  Backward with a fast form and a table that fits: its LAST
 * up256(64 * 4 n_types h d) bytes (up256: rounded up to 256) hold the 64 replicas of dR the row pass's workgroups add
 * into; with dR == NULL they are not touched. */
GRAPHOP_API int graphop_attention_etype_workspace_bytes(int dtype, int backward, int64_t n_edges, int64_t n_q, int64_t n_k,
                                            int64_t h, int64_t d, int64_t n_types, const graphop_plan_t* plan_r,
                                            const graphop_plan_t* plan_c, void* stream, int64_t* bytes_out);
GRAPHOP_API int graphop_attention_etype_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                    const int64_t* indices, const void* Q, const void* K, const void* V, const void* R,
                                    const int32_t* etype, void* o, void* stats, int64_t n_chunks, int64_t n_edges,
                                    int64_t n_q, int64_t n_k, int64_t h, int64_t d, int64_t n_types, void* workspace,
                                    int64_t workspace_bytes, const graphop_plan_t* plan, void* stream, double p,
                                    uint64_t seed, uint32_t offset, int64_t head0);
GRAPHOP_API int graphop_attention_etype_backward(int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                     const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                     const int64_t* eid_c, const int64_t* indices_c, const void* Q, const void* K,
                                     const void* V, const void* R, const int32_t* etype, const void* o, const void* stats,
                                     const void* dO, void* dQ, void* dK, void* dV, void* dR, int64_t n_row_chunks,
                                     int64_t n_col_chunks, int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h, int64_t d,
                                     int64_t n_types, void* workspace, int64_t workspace_bytes,
                                     const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream, double p,
                                     uint64_t seed, uint32_t offset, int64_t head0);

/* ---- an edge-type score bias in the fused attention step: <Q_i, K_j> + B[t_e, k] (ABI 8, additive; EXTRA ops) ---------
 * The step of graphop_attention_bias_* for a CATEGORICAL edge feature whose learned term is one scalar per (category,
 * head) inside the softmax: Graphormer's spatial encoding b_phi(i, j) (a shortest-path-distance bucket) and its edge
 * encoding on bond types, T5 / Swin-type bucketed relative-position biases, relation biases of heterogeneous graphs.
 * Edge e carries the type t_e = etype[e]; etype is (n_edges) int32, contiguous, indexed by EDGE ID, with values in
 * [0, n_types); B is (n_types, h) in the dtype of Q / K / V, contiguous and finite.  DESIGN.md 4.5p.
 *   s_e = <Q_i, K_j> + B[t_e, k]          one add, after the dot product's reduction
 *   every other line of graphop_attention_bias_* with b[e, k] := B[t_e, k]
 *   dB[t, k] = sum over the edges e with t_e = t of ds_e;  types no edge carries get dB[t] = 0
 * stats are those of the biased, undropped scores (graphop_attention_weights with b = B[etype] reproduces the weights);
 * rows without edges get o = 0 and stats = (-1e9, 0).  Nothing edge-sized is made in either direction: etype is the only
 * edge-sized operand.  Parallel edges share a dropout decision and may differ in type.  No 1 / sqrt(d) argument, and no
 * per-edge b, xe or R together with B.
 * OUT-OF-RANGE TYPES: etype is NOT scanned (a scan would synchronise the stream and break its capture in a graph).
 * Every kernel clamps the type it loads into [0, n_types - 1], as an unsigned value, before it forms an address: a type
 * outside [0, n_types) gives an undefined value (that of some type of the table) and never touches memory outside B / dB.
 * Arguments as graphop_attention_etype_* with B where R is and dB where dR is.  dB == NULL: the gradient of B is not
 * wanted; nothing is accumulated for it.  Otherwise the call itself writes every element of dB (as it zero-fills dQ, dK,
 * dV and what it accumulates into, with stream-ordered fills: a step can be captured).
 * Checks, all before anything touches a device: those of graphop_attention_forward, then the dropout arguments (head0
 * included), then n_types >= 1 (unless n_edges == 0), then B != NULL and etype != NULL (unless n_edges * h * d == 0),
 * then the workspace.  Empty problems fill what they must and dereference nothing.  A matching plan must bound the ids by
 * n_q and n_k (an error otherwise).
 * Forms, chosen pass by pass: fp32 calls whose (h, d) is one of (1,64) (2,32) (2,64) (4,16) (4,32) (4,64) (8,8) (8,16)
 * (8,32), with 16-byte aligned operands and ids below 2^31, run the chunk-driver passes k_attn_tbias_fwd_rows_f32 and
 * k_attn_tbias_bwd_rows_f32 under the conditions graphop_attention_etype_* puts on the plans.  The row pass with
 * dB != NULL sums dB in 4 n_types h bytes of LDS and so needs that to be at most 16 KiB (n_types * h <= 4096); beyond it
 * that pass alone is the generic one.  Everything else runs the generic kernels k_attn_tbias_*_generic, one wave per chunk.
 * workspace: graphop_attention_tbias_workspace_bytes bytes.  Backward with a fast form and a table that fits: its LAST
 * up256(64 * 4 n_types h) bytes (up256: rounded up to 256) hold the 64 replicas of dB the row pass's workgroups add
 * into; with dB == NULL they are not touched. */
GRAPHOP_API int graphop_attention_tbias_workspace_bytes(int dtype, int backward, int64_t n_edges, int64_t n_q, int64_t n_k,
                                            int64_t h, int64_t d, int64_t n_types, const graphop_plan_t* plan_r,
                                            const graphop_plan_t* plan_c, void* stream, int64_t* bytes_out);
GRAPHOP_API int graphop_attention_tbias_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                    const int64_t* indices, const void* Q, const void* K, const void* V, const void* B,
                                    const int32_t* etype, void* o, void* stats, int64_t n_chunks, int64_t n_edges,
                                    int64_t n_q, int64_t n_k, int64_t h, int64_t d, int64_t n_types, void* workspace,
                                    int64_t workspace_bytes, const graphop_plan_t* plan, void* stream, double p,
                                    uint64_t seed, uint32_t offset, int64_t head0);
GRAPHOP_API int graphop_attention_tbias_backward(int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                     const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                     const int64_t* eid_c, const int64_t* indices_c, const void* Q, const void* K,
                                     const void* V, const void* B, const int32_t* etype, const void* o, const void* stats,
                                     const void* dO, void* dQ, void* dK, void* dV, void* dB, int64_t n_row_chunks,
                                     int64_t n_col_chunks, int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h, int64_t d,
                                     int64_t n_types, void* workspace, int64_t workspace_bytes,
                                     const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream, double p,
                                     uint64_t seed, uint32_t offset, int64_t head0);

/* ---- attention weights of the fused dot-product attention ops (not in the reference) --------------
 * The weights the layer used, as an edge tensor (PyG's return_attention_weights=True, DGL's get_attention=True), from
 * the row statistics stats (n_q, h, 2) = (m_i, linv_i) that graphop_attention_forward / _dropout_forward /
 * _bias_forward / _edge_forward left.  Edge e = (i, j), head k; i indexes Q and stats, j indexes K; b, xe and a are
 * indexed by EDGE ID.  Three modes, chosen by which optional operand is given:
 *   plain:  s_e = <Q_i, K_j>                  b == NULL and xe == NULL
 *   bias :  s_e = <Q_i, K_j> + b[e]           b  (n_edges, h)
 *   edge :  s_e = <Q_i, K_j + xe[e]>          xe (n_edges, h, d); K_j + xe[e] formed once, as in attention_edge_forward
 *   a_e = exp(min(s_e - m_i, 0)) * linv_i     a  (n_edges, h), the edge layout of sparse_softmax / vector_spmm
 * a holds the UNDROPPED weights (the effective ones are a * graphop_edge_dropout_mask).  The min(..., 0) is deliberate:
 * the statistics may come from a kernel that summed the score in another order (the walk forward, the several-head
 * forward, a generic one), and the clamp keeps a_e <= linv_i <= 1 whichever forward made them.  b and xe together are an
 * error: no forward produces such statistics.  Rows without edges own no slot, so nothing is written for them.  a[e] is
 * written once for every edge id a row-major slot names; other entries are left untouched (zero-fill a first where the
 * chunk list may leave slots out).  No atomics and no workspace in any mode: the result is reproducible bit for bit.
 * Checks, all before anything touches a device, in this order: dtype and sizes; b and xe both given; stats or a NULL
 * (unless the problem is empty); a matching plan must bound the ids by n_q / n_k (an error, not a fall-back).  Empty
 * problems (n_chunks, n_edges, n_q, n_k or h * d zero) return OK and dereference nothing.
 * Forms: plain and bias are composed inside the library -- graphop_maskedmm_csr_forward (with a plan that covers every
 * edge id; else its _partial form, which fills nothing) writes s into a with the SDDMM driver its own dispatch picks, and
 * k_attn_weights_norm normalises a in place: one stream pass over (n_edges, h), any dtype, h, d, plan or chunk order.
 * Edge mode gathers: k_attn_weights_xe_f32 for fp32 calls whose (h, d) is one of (1,64) (2,32) (2,64) (4,16) (4,32)
 * (4,64) (8,8) (8,16) (8,32) with a matching plan, 16-byte aligned Q, K, stats, xe, a and ids below 2^31;
 * k_attn_weights_xe_generic (one wave per chunk) for everything else (fp64, other shapes, no plan, misaligned operands,
 * GRAPHOP_FORCE_GENERIC). */
GRAPHOP_API int graphop_attention_weights(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                              const int64_t* indices, const void* Q, const void* K, const void* stats, const void* b,
                              const void* xe, void* a, int64_t n_chunks, int64_t n_edges, int64_t n_q, int64_t n_k,
                              int64_t h, int64_t d, const graphop_plan_t* plan, void* stream);

/* ---- attention weights of the fused GAT and GATv2 layers (not in the reference) -------------------
 * The weights the layer used, as an edge tensor (PyG's return_attention_weights=True, DGL's get_attention=True), from
 * the row statistics stats (n_l, h, 2) = (m_i, linv_i) that graphop_gat_attention_forward / _dropout_forward /
 * graphop_gat_edge_attention_forward, or graphop_gatv2_attention_forward / _dropout_forward /
 * graphop_gatv2_edge_attention_forward, left.  Edge e = (i, j), head k; i indexes el / xl and stats, j indexes er / xr;
 * ee, xe and a are indexed by EDGE ID.  ee / xe == NULL: the layer without its edge operand.
 *   GAT  :  s_e = LeakyReLU((el[i,k] + er[j,k]) [+ ee[e,k]])                              ee (n_edges, h)
 *   GATv2:  s_e = sum_c att[k,c] * LeakyReLU((xl[i,k,c] + xr[j,k,c]) [+ xe[e,k,c]])       xe (n_edges, h, d)
 *   a_e = exp(min(s_e - m_i, 0)) * linv_i     a (n_edges, h), the edge layout of sparse_softmax / vector_spmm
 * The score is written with the expressions of the fused forwards.  a holds the UNDROPPED weights (the effective ones
 * are a * graphop_edge_dropout_mask).  The min(..., 0) is that of graphop_attention_weights: the statistics may come from
 * a kernel that summed in another order (the long-segment merge of the fused GATv2 forward, a generic kernel), and the
 * clamp keeps a_e <= linv_i <= 1 whichever forward made them.  a[e] is written once for every edge id a row-major slot
 * names; other entries are left untouched (zero-fill a first where the chunk list may leave slots out).  No atomics and
 * no workspace: the result is reproducible bit for bit.
 * Checks, all before anything touches a device, in this order: dtype and sizes; stats or a NULL (unless the problem is
 * empty); a matching plan must bound the ids by n_l / n_r (an error, not a fall-back).  Empty problems (n_chunks,
 * n_edges, n_l or n_r zero) return OK and dereference nothing.
 * Forms: k_gatw_f32 for fp32 calls with h in {1, 2, 4, 8}, a matching plan, ids below 2^31 and el, er, ee, a aligned to
 * 4 * min(h, 4) bytes (stats to 8); k_gv2w_f32 for fp32 calls whose (h, d) is one of (1,64) (2,32) (2,64) (4,16) (4,32)
 * (4,64) (8,8) (8,16) (8,32) with a matching plan, 16-byte aligned xl, xr, xe, att, stats, a and ids below 2^31; neither
 * owns a row, so any chunk order and partial chunk lists take them.  k_gatw_generic / k_gv2w_generic (one wave per chunk)
 * for everything else (fp64, other shapes, no plan, misaligned operands, GRAPHOP_FORCE_GENERIC). */
GRAPHOP_API int graphop_gat_attention_weights(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                              const int64_t* indices, const void* el, const void* er, const void* ee /* NULL ok */,
                              const void* stats, void* a, int64_t n_chunks, int64_t n_edges, int64_t n_l, int64_t n_r,
                              int64_t h, double negative_slope, const graphop_plan_t* plan, void* stream);
GRAPHOP_API int graphop_gatv2_attention_weights(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                              const int64_t* indices, const void* xl, const void* xr, const void* xe /* NULL ok */,
                              const void* att, const void* stats, void* a, int64_t n_chunks, int64_t n_edges,
                              int64_t n_l, int64_t n_r, int64_t h, int64_t d, double negative_slope,
                              const graphop_plan_t* plan, void* stream);

/* ---- halo pack / unpack of the node-range sharded step (not in the reference: single GPU) --------
 * gather_rows:      dst[i, :] = src[idx[i], :]          (send buffer of the rows peers gather from)
 * scatter_add_rows: dst[idx[i], :] += src[i, :]         (partial gradient rows coming home; idx may
 *                   repeat, native float atomics).  idx values must lie in [0, n_rows) (not checked:
 *                   the caller built them from its own range, custom_op_benchmark_amd/dist.py). */
GRAPHOP_API int graphop_gather_rows(int dtype, const void* src, const int64_t* idx, void* dst, int64_t n_idx,
                        int64_t n_src_rows, int64_t row_elems, void* stream);
/* add_rows_unique: the same as scatter_add_rows for an idx run WITHOUT repeats (the rows served to ONE
 * peer are distinct): plain read-add-write at streaming rate instead of memory-side atomics; runs for
 * different peers must be issued one after the other on the same stream. */
GRAPHOP_API int graphop_add_rows_unique(int dtype, const void* src, const int64_t* idx, void* dst, int64_t n_idx,
                            int64_t n_dst_rows, int64_t row_elems, void* stream);
GRAPHOP_API int graphop_scatter_add_rows(int dtype, const void* src, const int64_t* idx, void* dst, int64_t n_idx,
                             int64_t n_dst_rows, int64_t row_elems, void* stream);
/* add_rows_grouped (ABI 6): the received rows grouped by the own row they belong to --
 * dst[grp_rows[g], :] += sum over p in [grp_ptr[g], grp_ptr[g + 1]) of src[grp_pos[p], :] -- ONE launch for the
 * rows of all peers (add_rows_unique needs one per peer), every own row read and written once, no atomics,
 * fixed summation order.  grp_rows must hold distinct rows; the grouping is built once per shard (dist.py). */
GRAPHOP_API int graphop_add_rows_grouped(int dtype, const void* src, const int64_t* grp_ptr, const int64_t* grp_rows,
                             const int64_t* grp_pos, void* dst, int64_t n_groups, int64_t n_dst_rows,
                             int64_t row_elems, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GRAPHOP_HIP_H_ */
