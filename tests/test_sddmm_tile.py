"""Tile driver of the SDDMM-type passes (csrc/kernels_tile.h, csrc/tile_layout.h): a workgroup takes a (column window,
tile of R row pieces) task and gathers every neighbour row once per task.  Forced on small graphs through the tuning
knobs; maskedmm_csr_forward and the dedata of vector_spmm_backward against the oracle at the bounds of
tests/test_hip_parity.py, the way tests/test_walk.py checks the walk drivers.  The layout builder itself is checked
against brute force on the CPU (tests/test_sddmm_tile_host.py).

The second half of the file runs what sparse graphs under 32-KB windows never reach: tasks of several parts (dense rows),
column records that use all 14 offset bits (windows of 16384 ids), both sides of the automatic selection's two gates, the
scope gates under sddmm_tile = 2, the strips' results bit for bit, and outputs handed in full of NaN between guard bands.
Every one of those tests proves from the graph (tests/sddmm_tile_graphs.py) or from the plan's info record that it got
where it says, and fails otherwise; expected values come from the oracle alone."""
import contextlib
import ctypes
import functools
import types

import pytest
import torch

import oracle
from custom_op_benchmark_amd import _lib, graphs
from custom_op_benchmark_amd import graphop as ops
from gat_edge_reference import column_identity_edge_ids, permute_edge_ids
from sddmm_tile_graphs import (DESC_PARTS, MAX_WIN_COLS, dense_rows_graph, full_width_graph, pooled_graph, record_offsets,
                               repeated_pair_graph, task_parts_uncut, tile_cap)
from test_hip_parity import close
from util import random_graph

pytestmark = pytest.mark.gpu

TILE, STRIPS = "k_sddmm_tile_f32", "k_sddmm_wown_staged_f32"
TAGS = ("sddmm_fwd", "spmm_bwd_dedata")
D = 64


@pytest.fixture
def force_tile():
    _lib.tune_reset()
    _lib.tune("sddmm_tile", 2); _lib.tune("sddmm_tile_rows", 128)
    _lib.tune("sweep_min_kb", 0); _lib.tune("sweep_min_granule", 0); _lib.tune("window_kb", 32); _lib.tune("max_windows", 512)
    _lib.clear_plan_cache()
    yield
    _lib.tune_reset()
    _lib.clear_plan_cache()


def kernels_by_tag(step):
    _lib.profile_enable(True)
    step()
    torch.cuda.synchronize()
    k = {tag: r.get("kernel") for tag, r in _lib.profile_read().items()}
    _lib.profile_enable(False)
    return k


def check_both_passes(g, dev, seed, kernel=TILE):
    """maskedmm_csr_forward and vector_spmm_backward's dedata on the GPU against the oracle; which kernel ran."""
    gen = torch.Generator().manual_seed(seed)
    Q, dO = (torch.randn(g.n_src, D, generator=gen) / 8 for _ in range(2))
    K, V = (torch.randn(g.n_dst, D, generator=gen) / 8 for _ in range(2))
    a = torch.rand(g.n_edges, generator=gen)
    a8 = g.csr_args()
    want_s = oracle.maskedmm_csr_forward(g.row, g.ptr_r, g.eid_r, g.indices_r, Q, K)
    want_da = oracle.vector_spmm_backward(*a8, a, dO, V)[0]
    gd = g.to(dev)
    a8d = gd.csr_args()
    Qd, Kd, Vd, dOd, ad = (x.to(dev) for x in (Q, K, V, dO, a))
    # outputs start from garbage: every result must be written (the pass owes no zero fill to anyone)
    got = {}

    def step():
        got["s"] = ops.maskedmm_csr_forward(gd.row, gd.ptr_r, gd.eid_r, gd.indices_r, Qd, Kd)
        got["da"] = ops.vector_spmm_backward(*a8d, ad, dOd, Vd)[0]
    kern = kernels_by_tag(step)
    assert kern["sddmm_fwd"] == kernel and kern["spmm_bwd_dedata"] == kernel, kern
    close(got["s"], want_s)
    close(got["da"], want_da)
    return gd


def make_case(a8, n_src, n_dst, seed, h=1, d=D, dtype=torch.float32):
    """Inputs of both passes over the CSR pair a8 and the oracle's results for them (CPU), check_both_passes' draws at
    any (h, d, dtype).  Built once per graph and shared, unchanged, by the tests that use it (case())."""
    gen = torch.Generator().manual_seed(seed)
    ns = (lambda n: (n, d)) if h == 1 else (lambda n: (n, h, d))
    e = a8[2].numel()
    Q, dO = (torch.randn(*ns(n_src), generator=gen, dtype=dtype) / 8 for _ in range(2))
    K, V = (torch.randn(*ns(n_dst), generator=gen, dtype=dtype) / 8 for _ in range(2))
    a = torch.rand(*((e,) if h == 1 else (e, h)), generator=gen, dtype=dtype)
    return types.SimpleNamespace(a8=a8, n_src=n_src, n_dst=n_dst, n_edges=e, dtype=dtype, Q=Q, K=K, V=V, dO=dO, a=a,
                                 want_s=oracle.maskedmm_csr_forward(*a8[:4], Q, K),
                                 want_da=oracle.vector_spmm_backward(*a8, a, dO, V)[0])


def graph_case(g, seed, **kw):
    c = make_case(g.csr_args(), g.n_src, g.n_dst, seed, **kw)
    c.g = g
    return c


def not16_graph():
    g = random_graph(700, 700, 20000, seed=10, chunk_size=32)
    if g.n_edges % 16 == 0:
        g = graphs.graph_from_coo(g.src[:-3], g.dst[:-3], 700, 700, 32)
    assert g.n_edges % 16 != 0
    return g


CASES = {
    "g700": lambda: graph_case(random_graph(700, 700, 20000, seed=5, chunk_size=32), 21),
    "hub_row": lambda: graph_case(random_graph(700, 700, 20000, seed=7, chunk_size=32, hub=5000), 22),
    "not16": lambda: graph_case(not16_graph(), 23),
    # 400 x 1024, 800 / 300 columns per row drawn with replacement; 292 rows: a ragged last tile at 192 rows per tile;
    # 95 % of a row's columns in the lower half: what rows cut into pieces of 64 slots need to overfill a result buffer
    "dense800": lambda: graph_case(dense_rows_graph(400, 1024, 800, seed=31), 24),
    "dense300": lambda: graph_case(dense_rows_graph(400, 1024, 300, seed=32), 25),
    "dense_ragged": lambda: graph_case(dense_rows_graph(292, 1024, 800, seed=33), 26),
    "dense_skew": lambda: graph_case(dense_rows_graph(400, 1024, 800, seed=34, lo_share=0.95), 27),
    "long_rows": lambda: graph_case(dense_rows_graph(24, 1024, 14000, seed=36), 60),
    "long_rows_384": lambda: graph_case(dense_rows_graph(12, 1024, 28000, seed=37), 61),
    "full_width": lambda: graph_case(full_width_graph(1000, 4 * MAX_WIN_COLS, 40000, W=4, seed=35), 28),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@contextlib.contextmanager
def knobs(**kw):
    """force_tile's pattern for knob sets of a test's own: defaults, then kw, plan cache cleared; both restored."""
    _lib.tune_reset()
    defaults = _lib.tune_snapshot()
    for k, v in kw.items():
        _lib.tune(k, v)
    _lib.clear_plan_cache()
    try:
        yield defaults
    finally:
        _lib.profile_enable(False)
        _lib.tune_reset()
        _lib.clear_plan_cache()


FORCED = dict(sddmm_tile=2, sddmm_tile_rows=128, sweep_min_kb=0, sweep_min_granule=0, window_kb=32, max_windows=512)   # force_tile's


def run_case(c, dev):
    """Both passes of a case on the GPU -> (s, da, {tag: kernel}, the CSR pair on the device)."""
    a8d = tuple(x.to(dev) for x in c.a8)
    Qd, Kd, Vd, dOd, ad = (x.to(dev) for x in (c.Q, c.K, c.V, c.dO, c.a))
    got = {}

    def step():
        got["s"] = ops.maskedmm_csr_forward(*a8d[:4], Qd, Kd)
        got["da"] = ops.vector_spmm_backward(*a8d, ad, dOd, Vd)[0]
    kern = kernels_by_tag(step)
    assert all(t in kern for t in TAGS), kern
    return got["s"], got["da"], kern, a8d


def check_case(c, dev, kernel=TILE):
    """run_case, the kernel of both tags, both results against the oracle at the dtype's bound -> the row-major plan's info."""
    s, da, kern, a8d = run_case(c, dev)
    assert [kern[t] for t in TAGS] == [kernel, kernel], kern
    close(s, c.want_s, c.dtype)
    close(da, c.want_da, c.dtype)
    return plan_of(a8d, c).refresh_info(), a8d


def plan_of(a8d, c):
    return _lib.get_plan(*a8d[:4], c.n_dst)


def sweeps_of(plan):
    """[(W, win_cols, T, V)] of the window structures a plan holds."""
    out = []
    for i in range(_lib.lib().graphop_plan_n_sweeps(plan.handle)):
        si = _lib.SweepInfo()
        _lib.check(_lib.lib().graphop_plan_sweep_info(plan.handle, i, ctypes.byref(si)))
        out.append((int(si.W), int(si.win_cols), int(si.T), int(si.V)))
    return out


def with_edges(g, src, dst, n_src=None, n_dst=None):
    return graphs.graph_from_coo(torch.cat([g.src, src]), torch.cat([g.dst, dst]), n_src or g.n_src, n_dst or g.n_dst, 32)


@pytest.mark.parametrize("rows", [128, 192, 256, 384])
def test_tile_vs_oracle_every_tile_height(dev, force_tile, rows):
    """700 x 700, 20 k edges: several tiles with a ragged last one (700 = 5 x 128 + 60 = 3 x 192 + 124 = ...), eight
    windows; 128 / 192 rows run two workgroups of 512 threads per CU, 256 / 384 one of 1024."""
    _lib.tune("sddmm_tile_rows", rows)
    g = random_graph(700, 700, 20000, seed=5, chunk_size=32)
    gd = check_both_passes(g, dev, seed=rows)
    info = _lib.get_plan(gd.row, gd.ptr_r, gd.eid_r, gd.indices_r, g.n_dst).refresh_info()
    assert info.sddmm_tile_rows == rows and 0 < info.sddmm_tile_repeat_permille < 1000


def test_tile_hub_column_in_every_row(dev, force_tile):
    """One column sits in every row: its slots are split into records of four (groups of unequal length elsewhere)."""
    g = random_graph(700, 700, 20000, seed=6, chunk_size=32)
    g = with_edges(g, torch.arange(700), torch.full((700,), 233))
    check_both_passes(g, dev, seed=2)


def test_tile_hub_row_is_cut_into_pieces(dev, force_tile):
    """A row of 5,000 slots: dozens of row pieces, each with its share of every window."""
    g = random_graph(700, 700, 20000, seed=7, chunk_size=32, hub=5000)
    assert int(torch.bincount(g.src).max()) >= 5000
    check_both_passes(g, dev, seed=3)


def test_tile_empty_rows_and_empty_tasks(dev, force_tile):
    """30 % of the rows have no edge, and no edge reaches the last 200 columns: every tile's tasks in the last windows are empty."""
    g = random_graph(700, 500, 6000, seed=8, chunk_size=32, zero_rows=0.3)
    g = graphs.graph_from_coo(g.src, g.dst, 700, 700, 32)
    assert int(g.dst.max()) < 500
    check_both_passes(g, dev, seed=4)


@pytest.mark.parametrize("n_src,n_dst", [(300, 900), (900, 300)])
def test_tile_rectangular(dev, force_tile, n_src, n_dst):
    g = random_graph(n_src, n_dst, 9000, seed=9, chunk_size=32)
    check_both_passes(g, dev, seed=5)


def test_tile_edge_count_not_a_multiple_of_16(dev, force_tile):
    g = random_graph(700, 700, 20000, seed=10, chunk_size=32)
    if g.n_edges % 16 == 0:
        g = graphs.graph_from_coo(g.src[:-3], g.dst[:-3], 700, 700, 32)
    assert g.n_edges % 16 != 0
    check_both_passes(g, dev, seed=6)


def test_auto_keeps_the_strips_below_the_repeat_threshold(dev):
    """sddmm_tile = 1 (the default): 40,000 rows of ten edges over 40,000 columns in 64 windows make enough (window, tile)
    tasks for the grid, but a tile's 128 rows share hardly any neighbour inside a window -- the plan's repeat fraction is far below
    the threshold and the window-owner strips run."""
    _lib.tune_reset()
    _lib.tune("sddmm_tile_rows", 128); _lib.tune("sweep_min_granule", 0); _lib.tune("window_kb", 160)
    _lib.clear_plan_cache()
    try:
        assert _lib.tune_get("sddmm_tile") == 1
        g = random_graph(40000, 40000, 400000, seed=11, chunk_size=32)
        gd = check_both_passes(g, dev, seed=7, kernel=STRIPS)
        info = _lib.get_plan(gd.row, gd.ptr_r, gd.eid_r, gd.indices_r, g.n_dst).refresh_info()
        assert info.sddmm_tile_rows == 128                                     # the layout was analysed ...
        assert 0 < info.sddmm_tile_repeat_permille < 10 * _lib.tune_get("sddmm_tile_min_repeat")   # ... and found wanting
        _lib.tune("sddmm_tile", 2)                                             # the same plan, forced
        check_both_passes(g, dev, seed=7)
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()


def test_prepare_builds_the_tile_layout_and_the_pass_captures(dev, force_tile):
    """graphop.prepare builds the tile layout: the passes afterwards allocate nothing and synchronise nowhere, so they
    capture into a HIP graph (the queue heads are zeroed inside it) and the replay reproduces the eager results bit
    for bit -- every result is written exactly once, by plain stores."""
    g = random_graph(700, 700, 20000, seed=12, chunk_size=32, hub=900).to(dev)
    gen = torch.Generator(device=dev).manual_seed(8)
    Q, K, V, dO = (torch.randn(700, D, device=dev, generator=gen) / 8 for _ in range(4))
    a = torch.rand(g.eid_r.numel(), device=dev, generator=gen)
    ops.prepare(g, h=1, d=D, fused=False)
    held = _lib.plan_memory_bytes()
    a4, a8 = (g.row, g.ptr_r, g.eid_r, g.indices_r), g.csr_args()
    s0 = ops.maskedmm_csr_forward(*a4, Q, K)
    da0 = ops.vector_spmm_backward(*a8, a, dO, V)[0]
    assert _lib.plan_memory_bytes() == held            # the eager passes built nothing after prepare
    kern = kernels_by_tag(lambda: (ops.maskedmm_csr_forward(*a4, Q, K), ops.vector_spmm_backward(*a8, a, dO, V)))
    assert kern["sddmm_fwd"] == TILE and kern["spmm_bwd_dedata"] == TILE, kern
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = ops.maskedmm_csr_forward(*a4, Q, K)
        da = ops.vector_spmm_backward(*a8, a, dO, V)[0]
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(s, s0) and torch.equal(da, da0)


# ---- tasks of several parts ----------------------------------------------------------------------------------------------
# Two windows of 512 ids (sweep_w) and rows left whole (vrow_t above the longest row): a tile of R rows of some 400 slots per
# window overfills the result buffer (tile_cap(R) = 12032 / 7936 / 24064 / 15872 floats) several times over.
DENSE = dict(FORCED, sweep_w=2, vrow_t=1024)


def check_dense(c, dev, rows, vrow_t=1024):
    """A dense case with rows left whole, tile forced: both passes on the tile kernel against the oracle, the window
    structure the test reasons about (2 windows of 512 ids, one vrow per row), and the plan's part count against the
    greedy cut restated from the edge list (sddmm_tile_graphs.task_parts_uncut).  -> that [window, tile] part table."""
    assert int(torch.bincount(c.g.src).max()) <= vrow_t
    parts = task_parts_uncut(c.g, 2, rows, tile_cap(rows))
    with knobs(**dict(DENSE, sddmm_tile_rows=rows, vrow_t=vrow_t)):
        info, a8d = check_case(c, dev)
        assert sweeps_of(plan_of(a8d, c)) == [(2, 512, vrow_t, c.g.n_src)]
        assert info.sddmm_tile_rows == rows and info.sddmm_tile_max_parts == parts.max(), (info.sddmm_tile_max_parts, parts)
    return parts


@pytest.mark.parametrize("rows", [128, 192, 256, 384])
def test_tasks_of_many_parts_every_tile_height(dev, rows):
    """400 x 1024, 800 columns per row drawn with replacement (E = 320 k; duplicate pairs make records of several slots):
    a task of a full tile is cut into 5 to 11 parts, so the barrier behind the batch loop, the reset of the batch counter, the
    barrier before the buffer is reused and the write-out of a part that is not the first all run, and past the fourth
    part the part records come from global memory instead of LDS.  Proof of the path: the plan's sddmm_tile_max_parts
    equals the cut restated from the edge list, which is above kTileDescParts = 4 at every height; both tags ran the tile
    kernel."""
    parts = check_dense(case("dense800"), dev, rows)
    assert parts.max() > DESC_PARTS, parts


def test_tasks_of_two_to_four_parts(dev):
    """300 columns per row at 192 rows per tile: every part record of a task still comes through LDS (fetch_desc's 16
    ints), but the buffer is reused.  Proof: sddmm_tile_max_parts equals the restated cut, which is 2 .. 4."""
    parts = check_dense(case("dense300"), dev, 192)
    assert 2 <= parts.max() <= DESC_PARTS, parts


def test_ragged_last_tile_of_many_parts(dev):
    """292 rows at 192 per tile: the last tile has 100 rows, and its task in the last window -- the last task of the
    launch -- is cut into several parts.  Proof: the restated cut of that task, and sddmm_tile_max_parts equal to the
    restated maximum."""
    c = case("dense_ragged")
    assert c.g.n_src % 192 == 100
    parts = check_dense(c, dev, 192)
    assert parts.shape == (2, 2) and parts[1, 1] >= 2 and parts[1, 1] > DESC_PARTS, parts


@pytest.mark.parametrize("rows,name,vrow_t,n_parts", [(192, "long_rows", 16384, 24), (384, "long_rows_384", 32768, 12)])
def test_one_long_row_per_part(dev, rows, name, vrow_t, n_parts):
    """24 rows of 14000 columns drawn with replacement (12 of 28000 at 384 rows per tile), left whole: some 7000 (14000) slots
    per row and window, so at a buffer of 7936 (15872) floats every part is ONE row, and a task has 24 (12) of them.  A part's
    write-out is then the work of a single lane group, 440 (875) rounds of 16 floats, while the other 31 (63) groups have no
    row and stand at the barrier in front of the next part -- without that barrier they would put the next row's results
    into the buffer while this row's are still being copied out; the denser graphs above spread a part's write-out over
    some twenty groups of 25 rounds each, which is over before the first batch of the next part has its rows.  Result
    offsets and run lengths up to 14000 of their 16 bits.  Proof: the restated cut has one part per row in either task and
    equals sddmm_tile_max_parts; both tags ran the tile kernel."""
    parts = check_dense(case(name), dev, rows, vrow_t=vrow_t)
    assert parts.tolist() == [[n_parts], [n_parts]], parts


@pytest.mark.parametrize("touch", [0, 1])
def test_parts_that_begin_and_end_inside_a_row(dev, touch):
    """Rows of 800 slots cut into 13 pieces (vrow_t = 64), 95 % of a row's columns in the first of two windows: a piece holds
    59 slots there, a tile of 192 pieces 11 k -- two parts at a buffer of 7936 floats.  192 is no multiple of 13 and a part
    holds some 134 pieces, so tiles and parts begin and end inside rows.  With and without the L2 touches of the next
    task's streams (sddmm_tile_touch).  Proof: the window structure has 13 vrows per row, sddmm_tile_max_parts >= 2,
    both tags ran the tile kernel."""
    c = case("dense_skew")
    with knobs(**dict(FORCED, sddmm_tile_rows=192, sweep_w=2, vrow_t=64, sddmm_tile_touch=touch)):
        assert _lib.tune_get("sddmm_tile_touch") == touch
        info, a8d = check_case(c, dev)
        assert sweeps_of(plan_of(a8d, c)) == [(2, 512, 64, 13 * c.g.n_src)]
        assert info.sddmm_tile_rows == 192 and info.sddmm_tile_max_parts >= 2, info.sddmm_tile_max_parts


# ---- full-width windows --------------------------------------------------------------------------------------------------
def test_windows_of_16384_ids_use_every_offset_bit(dev):
    """1000 x 65536 under the default window_kb: four windows of 16384 ids, the widest a 16-bit column record addresses
    (14 bits of offset, 2 of slot count).  40 k uniform edges plus edges from five rows into the first id, the last id
    (offset 16383: every bit set) and the offsets 0x2AAA and 0x1555 of every window.  Proof: asserted from the edge list
    that each window holds all of those offsets and thousands at or above 8192; the plan's window structure is (4, 16384)."""
    c = case("full_width")
    w, off = record_offsets(c.g, 4)
    for wi in range(4):
        o = off[w == wi]
        assert all((o == x).any() for x in (0, MAX_WIN_COLS - 1, 0x2AAA, 0x1555)), wi
        assert int((o >= 8192).sum()) > 1000
    with knobs(sddmm_tile=2, sddmm_tile_rows=192, sweep_min_kb=0, sweep_min_granule=0) as defaults:
        assert defaults["window_kb"] == 4096 and _lib.tune_get("window_kb") == 4096
        info, a8d = check_case(c, dev)
        (W, win_cols, _, _), = sweeps_of(plan_of(a8d, c))
        assert (W, win_cols) == (4, MAX_WIN_COLS)
        assert info.sddmm_tile_rows == 192 and info.sddmm_tile_max_parts >= 1


# ---- automatic selection ---------------------------------------------------------------------------------------------------
def test_auto_takes_the_tile_kernel_above_both_gates_and_the_strips_below_the_task_gate(dev):
    """sddmm_tile = 1 and sddmm_tile_min_repeat as shipped.  384 rows per tile (one workgroup per CU) and 256 windows: the
    graph gets ceil(32 * n_cu / 256) tiles of rows, so W * tiles >= 32 * n_cu * per_cu holds with nothing to spare.  Every row
    has 24 edges and vrow_t = 64, so no row is cut and none is empty: V = n_src, which the window structure confirms.  A
    tile's rows draw from 48 columns of their own: nearly every slot repeats a neighbour of its task.  Proof of the positive
    side: the task product, sddmm_tile_repeat_permille >= 200, both tags on the tile kernel.  The same edges under 128
    windows halve the task product: the strips run, and the plan was not even analysed (the task gate stands in front of
    the layout count).  With test_auto_keeps_the_strips_below_the_repeat_threshold this holds both gates from both sides."""
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    R, W, n_dst = 384, 256, 32768
    tiles = -(-32 * n_cu // W)
    g = pooled_graph(tiles * R, n_dst, 24, R, 48, seed=41)
    assert int(torch.bincount(g.src, minlength=g.n_src).min()) == 24 == int(torch.bincount(g.src).max())
    c = graph_case(g, 29)
    common = dict(sddmm_tile_rows=R, max_windows=512, sweep_min_granule=0, vrow_t=64)
    with knobs(sweep_w=W, **common) as defaults:
        assert defaults["sddmm_tile"] == 1 == _lib.tune_get("sddmm_tile")
        assert defaults["sddmm_tile_min_repeat"] == 20 == _lib.tune_get("sddmm_tile_min_repeat")
        info, a8d = check_case(c, dev, TILE)
        assert sweeps_of(plan_of(a8d, c)) == [(W, n_dst // W, 64, g.n_src)]
        assert W * tiles >= 32 * n_cu > (W // 2) * tiles
        assert info.sddmm_tile_rows == R and info.sddmm_tile_repeat_permille >= 200, info.sddmm_tile_repeat_permille
    with knobs(sweep_w=W // 2, **common):
        assert _lib.tune_get("sddmm_tile") == 1
        info, a8d = check_case(c, dev, STRIPS)
        assert sweeps_of(plan_of(a8d, c)) == [(W // 2, 2 * n_dst // W, 64, g.n_src)]
        assert info.sddmm_tile_rows == 0 and info.sddmm_tile_repeat_permille == 0


# ---- scope gates -----------------------------------------------------------------------------------------------------------
def shuffled_chunks(g, seed):
    """The CSR pair of g with both chunk lists shuffled (row[] unsorted: the plan is not row-owned)."""
    gen = torch.Generator().manual_seed(seed)

    def shuffled(row, ptr):
        perm = torch.randperm(row.numel(), generator=gen)
        lens = (ptr[1:] - ptr[:-1])[perm]
        new_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
        slot = torch.cat([torch.arange(int(ptr[c]), int(ptr[c + 1])) for c in perm.tolist()])
        return row[perm].contiguous(), new_ptr, slot
    row, ptr_r, sr = shuffled(g.row, g.ptr_r)
    col, ptr_c, sc = shuffled(g.col, g.ptr_c)
    return (row, ptr_r, g.eid_r[sr].contiguous(), g.indices_r[sr].contiguous(),
            col, ptr_c, g.eid_c[sc].contiguous(), g.indices_c[sc].contiguous())


SCOPE = {   # name -> (case, extra knobs, a fact of the row-major plan's info that names the gate)
    "eid_column_identity": (lambda g: graph_case(column_identity_edge_ids(g)[0], 51), {}, ("eid_identity", 0)),
    "eid_permuted": (lambda g: graph_case(permute_edge_ids(g, 3)[0], 52), {}, ("eid_identity", 0)),
    "h4_d16": (lambda g: graph_case(g, 53, h=4, d=16), {}, ("eid_identity", 1)),
    "d32": (lambda g: graph_case(g, 54, d=32), {}, ("eid_identity", 1)),
    "d128": (lambda g: graph_case(g, 55, d=128), {}, ("eid_identity", 1)),
    "fp64": (lambda g: graph_case(g, 56, dtype=torch.float64), {}, ("eid_identity", 1)),
    "rows200": (lambda g: graph_case(g, 57), dict(sddmm_tile_rows=200), ("eid_identity", 1)),
    "shuffled_chunks": (lambda g: make_case(shuffled_chunks(g, 4), g.n_src, g.n_dst, 58), {}, ("row_owned", 0)),
}


@functools.lru_cache(maxsize=None)
def scope_case(name):
    return SCOPE[name][0](case("g700").g)


@pytest.mark.parametrize("name", list(SCOPE))
def test_out_of_scope_passes_fall_through_when_forced(dev, name):
    """sddmm_tile = 2 and the rest of force_tile on the 700 x 700 graph that test_tile_vs_oracle_every_tile_height runs on
    the tile kernel, each time with one thing outside the kernel's scope: edge ids that are the identity only in the
    column-major arrays, permuted edge ids, four heads, rows of 128 B and of 512 B, fp64, 200 rows per tile, shuffled chunk
    lists.  Both tags run their SDDMM over the ROW-major arrays and consult the row-major plan alone (launch_sddmm is
    handed the Csr `r` in graphop_vector_spmm_backward as in graphop_maskedmm_csr_forward; the column-major plan serves
    only the dx SpMM of the same call), so it is that plan's eid_identity / row_owned the case turns.  Proof: neither tag
    shows the tile kernel, the plan's info names the gate, and no tile layout was analysed (every scope gate stands in
    front of the layout count); results at the dtype's bound."""
    c = scope_case(name)
    _, extra, (field, value) = SCOPE[name]
    with knobs(**dict(FORCED, **extra)):
        s, da, kern, a8d = run_case(c, dev)
        assert TILE not in (kern[TAGS[0]], kern[TAGS[1]]), kern
        close(s, c.want_s, c.dtype)
        close(da, c.want_da, c.dtype)
        info = plan_of(a8d, c).refresh_info()
        assert getattr(info, field) == value
        assert info.sddmm_tile_rows == 0 and info.sddmm_tile_max_parts == 0


def test_a_row_piece_longer_than_the_buffer_keeps_the_strips(dev):
    """vrow_t is not clamped (graphop_hip.hip: choose_sweep takes the knob as it is), so a vrow may hold more slots inside
    one window than the result buffer: one (row, column) pair 9000 times under vrow_t = 16384 at 192 rows per tile (7936
    floats).  Forced and in scope, yet no layout exists (TileTotals::fits == false) and the strips run.  Proof: the row's
    length from the edge list, sddmm_tile_rows == 192 (the layout was counted) with sddmm_tile_max_parts == 0, both tags
    on the strips."""
    g = repeated_pair_graph(700, 700, 20000, row=77, column=300, times=9000, seed=13)
    assert int(((g.src == 77) & (g.dst == 300)).sum()) >= 9000 > tile_cap(192)
    c = graph_case(g, 59)
    with knobs(**dict(FORCED, sddmm_tile_rows=192, vrow_t=16384)):
        info, _ = check_case(c, dev, STRIPS)
        assert info.sddmm_tile_rows == 192 and info.sddmm_tile_max_parts == 0


# ---- bit for bit the strips' results ---------------------------------------------------------------------------------------
def ulps(a, b):
    """|a - b| in units of the last place (fp32, finite values)."""
    def ordered(x):
        i = x.detach().cpu().contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    return (ordered(a) - ordered(b)).abs()


BITWISE = {"g700": {}, "hub_row": {}, "dense800": dict(sddmm_tile_rows=192, sweep_w=2, vrow_t=1024)}


@pytest.mark.parametrize("name", list(BITWISE))
def test_tile_results_are_bitwise_the_strips(dev, name):
    """kernels_tile.h: "the same summation tree: a result is bitwise what the strips store".  Both passes once under
    sddmm_tile = 2 and once under sddmm_tile = 0 with the same window knobs, on the 700 x 700 graph, the hub-row graph and the
    dense graph whose tasks have ten parts: torch.equal on both results -- the slot -> (row, result offset) mapping has no
    tolerance to hide in.  Proof of the paths: the tile kernel on both tags in the first run, k_sddmm_wown_staged_f32 on
    both in the second."""
    c = case(name)
    with knobs(**dict(FORCED, **BITWISE[name])):
        s_t, da_t, kern, _ = run_case(c, dev)
        assert [kern[t] for t in TAGS] == [TILE, TILE], kern
    with knobs(**dict(dict(FORCED, **BITWISE[name]), sddmm_tile=0)):
        s_s, da_s, kern, _ = run_case(c, dev)
        assert [kern[t] for t in TAGS] == [STRIPS, STRIPS], kern
    for what, t, s, want in (("s", s_t, s_s, c.want_s), ("da", da_t, da_s, c.want_da)):
        close(t, want)
        close(s, want)
        u = ulps(t, s)
        print("%s %s: %d of %d results differ, at most %d ulp" % (name, what, int((u != 0).sum()), u.numel(), int(u.max())))
        assert torch.equal(t, s), what


# ---- every result written once, and nothing else ---------------------------------------------------------------------------
GUARD = 192   # floats on either side of the result: 768 B, so the result starts 16-byte aligned


def passes_into(c, dev, y_s, y_da):
    """Both passes through the C ABI, which takes the caller's outputs: s -> y_s, dedata -> y_da."""
    a8d = tuple(x.to(dev) for x in c.a8)
    Qd, Kd, Vd, dOd, ad = (x.to(dev) for x in (c.Q, c.K, c.V, c.dO, c.a))
    l, P = _lib.lib(), _lib.ptr
    plan_r, plan_c = _lib.get_plan(*a8d[:4], c.n_dst), _lib.get_plan(*a8d[4:], c.n_src)
    st = _lib.stream_of(Qd)
    dx = torch.empty_like(Vd)

    def step():
        _lib.check(l.graphop_maskedmm_csr_forward(_lib.F32, *(P(x) for x in a8d[:4]), P(Qd), P(Kd), P(y_s), a8d[0].numel(),
                                                  c.n_edges, c.n_src, c.n_dst, 1, D, plan_r.handle, st))
        _lib.check(l.graphop_vector_spmm_backward(_lib.F32, *(P(x) for x in a8d), P(ad), P(dOd), P(Vd), P(y_da), P(dx),
                                                  a8d[0].numel(), a8d[4].numel(), c.n_edges, c.n_dst, c.n_src, 1, D,
                                                  plan_r.handle, plan_c.handle, st))
    kern = kernels_by_tag(step)
    return kern, plan_r.refresh_info()


@pytest.mark.parametrize("name,min_parts", [("dense800", 2), ("not16", 1)])
def test_results_land_in_a_poisoned_buffer_and_nowhere_else(dev, name, min_parts):
    """Each pass writes into a view of E floats inside a larger buffer full of NaN, 192 floats of guard on either side, the
    view 16-byte aligned: afterwards every guard float is still NaN, no float of the view is, and the view meets the
    oracle -- every result written, none of them beside its place (a stray write inside the buffer lands in a guard
    band).  On the dense graph (ten parts per task at 192 rows per tile) and on the graph whose edge count is no multiple
    of 16.  Proof: both tags on the tile kernel, sddmm_tile_max_parts."""
    c = case(name)
    extra = dict(sddmm_tile_rows=192, sweep_w=2, vrow_t=1024) if name == "dense800" else {}
    with knobs(**dict(FORCED, **extra)):
        bufs = [torch.full((c.n_edges + 2 * GUARD,), float("nan"), device=dev) for _ in range(2)]
        views = [b[GUARD:GUARD + c.n_edges] for b in bufs]
        assert all(v.data_ptr() % 16 == 0 and v.numel() == c.n_edges for v in views)
        kern, info = passes_into(c, dev, *views)
        assert [kern[t] for t in TAGS] == [TILE, TILE], kern
        assert info.sddmm_tile_max_parts >= min_parts
        for b, v, want in zip(bufs, views, (c.want_s, c.want_da)):
            assert bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[GUARD + c.n_edges:]).all())
            assert not bool(torch.isnan(v).any())
            close(v, want)
