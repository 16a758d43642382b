"""Tile driver of the SDDMM-type passes (csrc/kernels_tile.h, csrc/tile_layout.h): a workgroup takes a (column window,
tile of R row pieces) task and gathers every neighbour row once per task.  Forced on small graphs through the tuning
knobs; maskedmm_csr_forward and the dedata of vector_spmm_backward against the oracle at the bounds of
tests/test_hip_parity.py, the way tests/test_walk.py checks the walk drivers.  The layout builder itself is checked
against brute force on the CPU (tests/test_sddmm_tile_host.py)."""
import pytest
import torch

import oracle
from custom_op_benchmark_amd import _lib, graphs
from custom_op_benchmark_amd import graphop as ops
from test_hip_parity import close
from util import random_graph

pytestmark = pytest.mark.gpu

TILE, STRIPS = "k_sddmm_tile_f32", "k_sddmm_wown_staged_f32"
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
