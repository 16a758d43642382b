"""GPU tier of the attention dropout of the fused GATv2 layer: graphop.gatv2_attention_dropout_forward / _backward,
functions.FusedGATv2AttentionDropout and the two dropout steps against the float64 reference of
tests/gatv2_dropout_reference.py, against each other and against the undropped ops at p = 0.

Bounds (none new): o, stats, dxl, dxr at rtol = 1e-4 / atol = 1e-5 / (1 - p) against float64 (1e-10 / 1e-10 in fp64); datt
at |err| <= K * S with S from the dropout reference, K = 1e-6 (1e-12 in fp64).  Every measured ratio is printed.
Measured on an MI355X: o, stats, dxl, dxr at most 0.07 / 0.03 / 0.33 / 0.14 of their bound in fp32 (dxl: the generic kernels
at (8, 32) on the 20k-node graph) and 2.2e-4 of it in fp64; datt at most 1.4e-7 * S in fp32 (the graph with rows of up to
5000 slots) and 3.6e-16 * S in fp64; the fused against the composed dropout step at most 0.08 of twice the bound."""
import functools

import pytest
import torch

import dropout_reference as DR
import fused_gatv2_reference as R
import gatv2_dropout_reference as RD
from custom_op_benchmark_amd import _lib, functions, graphop as ops, graphs
from gat_reference import reorder_chunks
from test_gat_dropout import _unsplit_graph
from test_gat_launch_geometry import (BLOCK, MAX_ROW_BLOCKS, _assert_cpg, _cpg, _geometry, _graph, _grid, _on_device,
                                      _shuffled, _sweep_key)
from util import random_graph

pytestmark = pytest.mark.gpu

SLOPE = 0.2
SEED, OFFSET = 1234567890123, 7
FAST_NAMES = {"gv2attn_drop_fwd": "k_gv2attn_drop_fwd_f32", "gv2attn_pack": "k_gv2attn_pack_f32",
              "gv2attn_drop_bwd_row": "k_gv2attn_drop_bwd_row_f32", "gv2attn_drop_bwd_col": "k_gv2attn_drop_bwd_col_f32",
              "gv2attn_datt_fin": "k_gv2attn_datt_fin_f32"}
GENERIC_NAMES = {"gv2attn_drop_fwd": "k_gv2attn_drop_fwd_generic", "gv2attn_pack": "k_gv2attn_pack_generic",
                 "gv2attn_drop_bwd_row": "k_gv2attn_drop_bwd_row_generic",
                 "gv2attn_drop_bwd_col": "k_gv2attn_drop_bwd_col_generic"}
UNDROPPED_FAST = {"gv2attn_fwd": "k_gv2attn_fwd_f32", "gv2attn_pack": "k_gv2attn_pack_f32",
                  "gv2attn_bwd_row": "k_gv2attn_bwd_row_f32", "gv2attn_bwd_col": "k_gv2attn_bwd_col_f32",
                  "gv2attn_datt_fin": "k_gv2attn_datt_fin_f32"}
OUT = ("o", "stats", "dxl", "dxr")


def _profiled(fn):
    """-> (fn(), {tag: kernel name} of what it launched)"""
    _lib.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        prof = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    return out, {tag: rec["kernel"] for tag, rec in prof.items() if tag.startswith("gv2attn_")}


def _run(a8, dev, x, p, seed=SEED, offset=OFFSET, slope=SLOPE):
    """(o, stats, dxl, dxr, datt) through graphop.gatv2_attention_dropout_forward / _backward, and the kernels launched"""
    xl, xr, att, dO = (t.to(dev) for t in x)

    def go():
        o, stats = ops.gatv2_attention_dropout_forward(*a8[:4], xl, xr, att, slope, p, seed, offset)
        return [o, stats] + ops.gatv2_attention_dropout_backward(*a8, xl, xr, att, o, stats, dO, slope, p, seed, offset)
    return _profiled(go)


def _check(got, want, what, p, dtype=torch.float32, scale=1.0):
    """got = (o, stats, dxl, dxr, datt) on the device, want = RD.reference(...); scale = 2 where got is held against
    another fp32 result that is itself inside the bound (an entry of want that it does not have is None: not compared)"""
    tol, K = RD.tol(dtype, p)
    tol, K = dict(rtol=tol["rtol"] * scale, atol=tol["atol"] * scale), K * scale
    pairs = [(name, x, y) for name, x, y in zip(OUT, got, want) if y is not None]
    for name, x, y in pairs:
        assert x.dtype == dtype and x.shape == y.shape, (what, name, x.dtype, x.shape, y.shape)
        print("%s %s: %.3g of the bound" % (what, name, R.ratio(x, y, tol)))
    r = R.datt_ratio(got[4], want[4], want[5])
    print("%s datt: max |err| / S = %.3g (bound %.1g)" % (what, r, K))
    for name, x, y in pairs:
        torch.testing.assert_close(x.cpu().double(), y.cpu().double(), **tol,
                                   msg=lambda m: "%s %s: %s" % (what, name, m))
    assert got[4].dtype == dtype and got[4].shape == want[4].shape
    assert r <= K, "%s datt: max |err| / S = %g" % (what, r)


# ---- 1. the float64 reference on the irregular graph ------------------------------------------------------------------
@pytest.mark.parametrize("chunk_size", [3, 32])
@pytest.mark.parametrize("h,d", [(1, 64), (1, 8), (2, 32), (3, 8), (4, 16), (8, 8), (8, 16), (8, 32)])
def test_fused_gatv2_dropout_matches_the_float64_reference(dev, h, d, chunk_size):
    """A fifth of the rows empty, one hub row of parallel edges above the 1024-slot long-segment bound; fast and generic
    shapes, fp32 and fp64, p in {0.1, 0.5, 0.6} and 0.9 in fp64.  At p = 0.6, h = 1, seed = offset = 0 some non-empty
    rows lose every edge: their o and dxl rows from the device are exactly zero."""
    g = R.irregular_graph(chunk_size)
    deg = torch.bincount(g.src, minlength=g.n_src)
    assert int(deg.max()) > 1024 and torch.unique(torch.stack([g.src, g.dst], 1), dim=0).size(0) < g.n_edges
    gd = g.to(dev)
    for p in (0.1, 0.5, 0.6, 0.9):
        seed, offset = (0, 0) if p == 0.6 else (SEED, OFFSET)
        for dtype in (torch.float32, torch.float64) if p < 0.9 else (torch.float64,):
            x = R.inputs(g, h, d, seed=h + d + chunk_size, dtype=dtype)
            want = RD.reference(g, *x, SLOPE, p, seed, offset)
            got, names = _run(gd.csr_args(), dev, x, p, seed, offset)
            fast = dtype == torch.float32 and (h, d) in R.FAST
            assert names == (FAST_NAMES if fast else GENERIC_NAMES), names
            empty = deg == 0
            assert not got[0].cpu()[empty].any() and bool((got[1].cpu()[empty][..., 0] == -1e9).all())
            _check(got, want, "(%d, %d) chunk %d p=%g %s" % (h, d, chunk_size, p, str(dtype)[6:]), p, dtype)
            if p == 0.6 and h == 1:
                gone = DR.fully_dropped_rows(g.src, g.dst, g.n_src, 1, p, seed, offset)[:, 0]
                assert int(gone.sum()) == {3: 6, 32: 4}[chunk_size]
                assert not got[0].cpu()[gone].any() and not got[2].cpu()[gone].any()
                assert bool((got[1].cpu()[gone][..., 1] > 0).all())        # ... and its stats are those of its scores


# ---- 2. row lengths around the batch and long-segment edges --------------------------------------------------------
@pytest.mark.parametrize("h,d", [(1, 64), (4, 32), (8, 32)])
def test_fused_gatv2_dropout_row_lengths_at_the_batch_and_long_segment_edges(dev, h, d):
    """Rows of exactly 1, SB - 1, SB, SB + 1, 1024, 1025, 2049 and 5000 slots at p = 0.5: slots past the end of a batch
    keep weight 0 whatever their keep bits say, the long-segment merge is unchanged, and stats are bit for bit those of
    the undropped forward."""
    g = R.edge_rows_graph()
    gd = g.to(dev)
    x = R.inputs(g, h, d, seed=h * 100 + d)
    got, names = _run(gd.csr_args(), dev, x, 0.5)
    assert names == FAST_NAMES, names
    _check(got, RD.reference(g, *x, SLOPE, 0.5, SEED, OFFSET), "edge rows (%d, %d)" % (h, d), 0.5)
    xl, xr, att, _ = (t.to(dev) for t in x)
    o0, stats0 = ops.gatv2_attention_forward(*gd.csr_args()[:4], xl, xr, att, SLOPE)
    assert torch.equal(got[1], stats0) and not torch.equal(got[0], o0)


# ---- 3. rectangular graph, shuffled chunk lists ------------------------------------------------------------------------
def test_fused_gatv2_dropout_shuffled_chunks_rectangular(dev):
    """Chunks in random order on both orientations, n_src != n_dst: the forward takes its generic form (no row_owned
    plan), the backward its fast OWNED = false forms; (i, j) keeps its order in the column-major pass."""
    g = random_graph(260, 190, 5000, seed=11, chunk_size=8, zero_rows=0.2, hub=500)
    gen = torch.Generator().manual_seed(1)
    pr = reorder_chunks(g.ptr_r, g.row, g.eid_r, g.indices_r, torch.randperm(g.n_row_chunks, generator=gen))
    pc = reorder_chunks(g.ptr_c, g.col, g.eid_c, g.indices_c, torch.randperm(g.n_col_chunks, generator=gen))
    csr = tuple(t.to(dev) for t in (pr[1], pr[0], pr[2], pr[3], pc[1], pc[0], pc[2], pc[3]))
    for plan in (_lib.get_plan(*csr[:4], g.n_dst), _lib.get_plan(*csr[4:], g.n_src)):
        assert not plan.info.row_owned and not plan.info.rows_sorted
    assert g.n_src != g.n_dst
    for h, d, dtype in ((4, 16, torch.float32), (8, 8, torch.float32), (3, 8, torch.float64)):
        x = R.inputs(g, h, d, seed=h, dtype=dtype)
        got, names = _run(csr, dev, x, 0.6, 99, 3)
        if dtype == torch.float32:
            assert names == dict(FAST_NAMES, gv2attn_drop_fwd="k_gv2attn_drop_fwd_generic"), names
        else:
            assert names == GENERIC_NAMES, names
        _check(got, RD.reference(g, *x, SLOPE, 0.6, 99, 3), "shuffled (%d, %d)" % (h, d), 0.6, dtype)


# ---- 4. every fast shape: composed step, planned, NULL plan -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chung_lu():
    return graphs.chung_lu_graph(20000, 200000, alpha=0.5, seed=1)


def _c_abi(g, dev, xl, xr, att, dO, p, plan_r, plan_c):
    """One forward + backward through the C ABI with the given plan handles (None: plan = NULL)"""
    P, l, st = _lib.ptr, _lib.lib(), _lib.stream_of(xl)
    h, d = (1, xl.size(1)) if xl.dim() == 2 else (xl.size(1), xl.size(2))
    o, stats = torch.empty_like(xl), torch.empty((g.n_src, h, 2), device=dev)
    dxl, dxr, datt = torch.empty_like(xl), torch.empty_like(xr), torch.empty_like(att)
    ws = torch.empty(max(ops._gatv2_attention_workspace_values(g.n_src, g.n_row_chunks, h, d), 1), device=dev)
    _lib.check(l.graphop_gatv2_attention_dropout_forward(
        _lib.F32, P(g.row), P(g.ptr_r), P(g.eid_r), P(g.indices_r), P(xl), P(xr), P(att), P(o), P(stats), g.n_row_chunks,
        g.n_edges, g.n_src, g.n_dst, h, d, SLOPE, p, SEED, OFFSET, plan_r, st))
    _lib.check(l.graphop_gatv2_attention_dropout_backward(
        _lib.F32, *(P(t) for t in g.csr_args()), P(xl), P(xr), P(att), P(o), P(stats), P(dO), P(dxl), P(dxr), P(datt),
        P(ws), ws.numel() * 4, g.n_row_chunks, g.n_col_chunks, g.n_edges, g.n_src, g.n_dst, h, d, SLOPE, p, SEED, OFFSET,
        plan_r, plan_c, st))
    return [o, stats, dxl, dxr, datt]


@pytest.mark.parametrize("h,d", R.FAST)
def test_fused_gatv2_dropout_every_fast_shape_composed_planned_and_null_plan(dev, h, d):
    """p = 0.6 on a 20k-node Chung-Lu graph: the fused dropout step against gatv2_attention_dropout_step (two fp32
    results, each inside the bound: twice the bound between them), the C ABI with plans (fast kernels) and with
    plan = NULL (generic kernels) inside the bounds of the float64 reference; two planned runs give bit-equal o, stats
    and datt."""
    p = 0.6
    g0 = _chung_lu()
    g = g0.to(dev)
    x = R.inputs(g0, h, d, seed=h * 100 + d)
    xl, xr, att, dO = (t.to(dev) for t in x)
    plan_r = _lib.get_plan(g.row, g.ptr_r, g.eid_r, g.indices_r, g.n_dst)
    plan_c = _lib.get_plan(g.col, g.ptr_c, g.eid_c, g.indices_c, g.n_src)
    want = RD.reference(g0, *x, SLOPE, p, SEED, OFFSET)
    planned, names = _profiled(lambda: _c_abi(g, dev, xl, xr, att, dO, p, plan_r.handle, plan_c.handle))
    assert names == FAST_NAMES, names
    again = _c_abi(g, dev, xl, xr, att, dO, p, plan_r.handle, plan_c.handle)
    for i in (0, 1, 4):
        assert torch.equal(planned[i], again[i]), "run-to-run difference in %s" % (OUT + ("datt",))[i]
    unplanned, names = _profiled(lambda: _c_abi(g, dev, xl, xr, att, dO, p, None, None))
    assert names == GENERIC_NAMES, names
    _check(planned, want, "planned (%d, %d)" % (h, d), p)
    _check(unplanned, want, "NULL plan (%d, %d)" % (h, d), p)
    leaves = [t.clone().requires_grad_(True) for t in (xl, xr, att)]
    o = functions.fused_gatv2_attention_dropout_step(g, *leaves, dO, p, SEED, OFFSET, SLOPE)
    torch.cuda.synchronize()
    fused = [o.detach(), planned[1]] + [t.grad for t in leaves]
    _check(fused, want, "fused step (%d, %d)" % (h, d), p)
    assert torch.equal(o.detach(), planned[0])
    leaves2 = [t.clone().requires_grad_(True) for t in (xl, xr, att)]
    _, a, o2 = functions.gatv2_attention_dropout_step(g, *leaves2, dO, p, SEED, OFFSET, SLOPE)
    torch.cuda.synchronize()
    assert a.shape[0] == g.n_edges and bool((a > 0).all())                   # the weights it returns are the undropped ones
    composed = [o2.detach().cpu(), None] + [t.grad.cpu() for t in leaves2]      # (the composed step has no stats)
    _check(fused, composed + [want[5]], "fused vs composed (%d, %d)" % (h, d), p, scale=2.0)


# ---- 5. p = 0 is the undropped op -------------------------------------------------------------------------------------
def test_fused_gatv2_dropout_p_zero_is_the_undropped_op(dev):
    """p = 0 runs the undropped kernels under the undropped tags.  On a graph where no row or column is split nothing is
    summed by atomics except the generic row pass's datt (one add per chunk and element, in any order): everything else
    is bit-equal."""
    for gseed in (3, 32):
        g0 = _unsplit_graph(gseed)
        g = g0.to(dev)
        a8 = g.csr_args()
        for h, d, dtype in ((1, 64, torch.float32), (8, 8, torch.float32), (3, 8, torch.float32),
                            (2, 4, torch.float64)):
            xl, xr, att, dO = (t.to(dev) for t in R.inputs(g0, h, d, seed=h, dtype=dtype))
            f0 = ops.gatv2_attention_forward(*a8[:4], xl, xr, att, SLOPE)
            b0 = ops.gatv2_attention_backward(*a8, xl, xr, att, *f0, dO, SLOPE)

            def go():
                f1 = ops.gatv2_attention_dropout_forward(*a8[:4], xl, xr, att, SLOPE, 0.0, 77, 5)
                return f1 + ops.gatv2_attention_dropout_backward(*a8, xl, xr, att, *f0, dO, SLOPE, 0.0, 77, 5)
            got, names = _profiled(go)
            fast = dtype == torch.float32 and (h, d) in R.FAST
            assert not [t for t in names if "drop" in t or "drop" in names[t]], names
            assert (names == UNDROPPED_FAST) if fast else ("gv2attn_fwd" in names and "gv2attn_bwd_col" in names), names
            for i, (u, v) in enumerate(zip(f0 + b0, got)):
                if i == 4 and not fast:
                    torch.testing.assert_close(u, v, **(R.TOL32 if dtype == torch.float32 else R.TOL64))
                else:
                    assert torch.equal(u, v), (h, d, dtype, i)
    # a graph with split rows: atomics in any order, inside the tolerances of the reference
    g0 = R.irregular_graph(3)
    g = g0.to(dev)
    for h, d in ((4, 16), (3, 8)):
        x = R.inputs(g0, h, d, seed=h)
        got, names = _run(g.csr_args(), dev, x, 0.0, 77, 5)
        assert not [t for t in names if "drop" in t], names
        want = R.reference(g0, *x, SLOPE)
        _check(got, want[:6], "p = 0 hub graph (%d, %d)" % (h, d), 0.0)


# ---- 6. repeatability -------------------------------------------------------------------------------------------------
def test_fused_gatv2_dropout_is_repeatable_and_depends_on_seed_and_offset(dev):
    g0 = _unsplit_graph(3)
    g = g0.to(dev)
    a8 = g.csr_args()
    for h, d in ((1, 64), (8, 16), (3, 8)):
        x = R.inputs(g0, h, d, seed=h)
        run = lambda seed, off: _run(a8, dev, x, 0.5, seed, off)[0]
        a, b, c, e = run(11, 0), run(11, 0), run(11, 1), run(12, 0)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert not torch.equal(a[0], c[0]) and not torch.equal(a[0], e[0])
        assert torch.equal(a[1], c[1]) and torch.equal(a[1], e[1])            # the stats do not see the dropout
    # the autograd class: seed=None draws from torch's default CPU generator
    xl, xr, att, _ = (t.to(dev) for t in x)
    outs = []
    for _ in range(2):
        torch.manual_seed(5)
        outs.append(functions.FusedGATv2AttentionDropout.apply(*a8, xl, xr, att, SLOPE, 0.5, None, 0))
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[0], functions.FusedGATv2AttentionDropout.apply(*a8, xl, xr, att, SLOPE, 0.5, None, 0))


# ---- 7. autograd ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,d", [(1, 3), (2, 4)])
def test_fused_gatv2_dropout_gradcheck(dev, h, d):
    g = random_graph(12, 10, 50, seed=4, chunk_size=3, hub=8).to(dev)
    gen = torch.Generator().manual_seed(0)
    xl = torch.randn(R.node_shape(g.n_src, h, d), generator=gen, dtype=torch.float64).to(dev).requires_grad_(True)
    xr = torch.randn(R.node_shape(g.n_dst, h, d), generator=gen, dtype=torch.float64).to(dev).requires_grad_(True)
    att = torch.randn(R.node_shape(1, h, d)[1:], generator=gen, dtype=torch.float64).to(dev).requires_grad_(True)
    assert torch.autograd.gradcheck(
        lambda a, b, c: functions.FusedGATv2AttentionDropout.apply(*g.csr_args(), a, b, c, SLOPE, 0.5, 42, 3),
        (xl, xr, att), nondet_tol=1e-12)   # (split rows are summed by float atomics: the order of the adds may differ)


def test_fused_gatv2_dropout_function_saves_no_edge_tensor(dev):
    g = random_graph(60, 50, 900, seed=8, chunk_size=8).to(dev)
    xl, xr, att, dO = (t.to(dev) for t in R.inputs(g, 4, 16, seed=1))
    xl, xr, att = (t.requires_grad_(True) for t in (xl, xr, att))
    o = functions.FusedGATv2AttentionDropout.apply(*g.csr_args(), xl, xr, att, SLOPE, 0.5, 42, 3)
    saved = o.grad_fn.saved_tensors
    assert len(saved) == 13 and [t.data_ptr() for t in saved[8:11]] == [xl.data_ptr(), xr.data_ptr(), att.data_ptr()]
    assert all(t.size(0) != g.n_edges for t in saved[8:]) and saved[12].shape == (g.n_src, 4, 2)
    o.backward(dO)
    want = ops.gatv2_attention_dropout_backward(*g.csr_args(), xl.detach(), xr.detach(), att.detach(), o.detach(),
                                                saved[12], dO, SLOPE, 0.5, 42, 3)
    for got, w in zip((xl.grad, xr.grad, att.grad), want):
        torch.testing.assert_close(got, w, rtol=1e-4, atol=2e-5)


# ---- 8. bindings and messages --------------------------------------------------------------------------------------------
def test_fused_gatv2_dropout_bindings_agree(dev):
    ext = ops.cpp_ext
    assert ext is not None, "graphop_cpp.so not built (run __graft_entry__.build())"
    g0 = random_graph(500, 400, 8000, seed=6, chunk_size=32, hub=900)
    g = g0.to(dev)
    a8 = g.csr_args()
    dr = (0.6, 2 ** 63 - 1, 2 ** 32 - 1)
    for h, d in ((1, 64), (4, 16), (3, 5)):
        xl, xr, att, dO = (x.to(dev) for x in R.inputs(g0, h, d, seed=h))
        f0 = ops.gatv2_attention_dropout_forward(*a8[:4], xl, xr, att, -0.1, *dr)
        f1 = ext.gatv2_attention_dropout_forward(*a8[:4], xl, xr, att, -0.1, *dr)
        f2 = torch.ops.graphop.gatv2_attention_dropout_forward(*a8[:4], xl, xr, att, -0.1, *dr)
        assert len(f0) == len(f1) == len(f2) == 2
        for u, v, w in zip(f0, f1, f2):
            if (h, d) in R.FAST:      # the fast forward uses no atomics: one result, bit for bit
                assert torch.equal(u, v) and torch.equal(u, w)
            torch.testing.assert_close(u, v, rtol=1e-4, atol=1e-5 / (1 - dr[0]))
            torch.testing.assert_close(u, w, rtol=1e-4, atol=1e-5 / (1 - dr[0]))
        want = RD.reference(g0, *(t.cpu() for t in (xl, xr, att, dO)), -0.1, *dr)
        b0 = ops.gatv2_attention_dropout_backward(*a8, xl, xr, att, *f0, dO, -0.1, *dr)
        b1 = ext.gatv2_attention_dropout_backward(*a8, xl, xr, att, *f0, dO, negative_slope=-0.1, p=dr[0], seed=dr[1],
                                                  offset=dr[2])
        b2 = torch.ops.graphop.gatv2_attention_dropout_backward(*a8, xl, xr, att, *f0, dO, -0.1, *dr)
        assert len(b0) == len(b1) == len(b2) == 3
        for b in (b0, b1, b2):
            _check(f0 + b, want, "bindings (%d, %d)" % (h, d), dr[0])
    with pytest.raises(RuntimeError, match="same h"):
        ops.gatv2_attention_dropout_forward(*a8[:4], xl, xr[:, :2].contiguous(), att, 0.2, 0.5)
    with pytest.raises(RuntimeError, match="same dtype"):
        ops.gatv2_attention_dropout_forward(*a8[:4], xl, xr, att.double(), 0.2, 0.5)
    for op in (ops.gatv2_attention_dropout_backward, torch.ops.graphop.gatv2_attention_dropout_backward):
        with pytest.raises(RuntimeError, match="o must be"):
            op(*a8, xl, xr, att, f0[0][:, :2].contiguous(), f0[1], dO, 0.2, 0.5)
        with pytest.raises(RuntimeError, match="dO must match"):
            op(*a8, xl, xr, att, *f0, dO[:10].contiguous(), 0.2, 0.5)
        with pytest.raises(RuntimeError, match="same dtype"):
            op(*a8, xl, xr, att, *f0, dO.double(), 0.2, 0.5)


# ---- 9. the launch geometry of large graphs -----------------------------------------------------------------------------
P_GEO = 0.3


@functools.lru_cache(maxsize=None)
def _geometry_case(key, h, d):
    g = _graph(*key)
    x = R.inputs(g, h, d, seed=h * 100 + d + 3)
    return x, RD.reference(g, *x, SLOPE, P_GEO, SEED, OFFSET)


@pytest.mark.parametrize("hd", [(1, 64), (8, 32)])
@pytest.mark.parametrize("cpg", [2, 16])
def test_fused_gatv2_dropout_at_cpg(dev, cpg, hd):
    """The dropout kernels with 2 and 16 chunks per lane group: the row-change branch, the plain store of a node inside a
    group and the clipped last group all run; one Philox block per slot at (1, 64), two (one per lane) at (8, 32)."""
    key = _sweep_key(dev, cpg)
    g = _on_device(key, str(dev))
    _assert_cpg(g, dev, 16, cpg)
    x, want = _geometry_case(key, *hd)
    got, names = _run(g.csr_args(), dev, x, P_GEO)
    assert names == FAST_NAMES, names
    _check(got, want, "cpg=%d %s" % (cpg, hd), P_GEO)


def test_fused_gatv2_dropout_unordered_chunks_at_cpg(dev):
    """Chunk lists in random order at cpg >= 3, (4, 32): the OWNED = false forms of both backward passes."""
    key, csr = _shuffled(dev)
    x, want = _geometry_case(key, 4, 32)
    got, names = _run(csr, dev, x, P_GEO)
    assert names == dict(FAST_NAMES, gv2attn_drop_fwd="k_gv2attn_drop_fwd_generic"), names
    _check(got, want, "unordered (4, 32)", P_GEO)


def test_fused_gatv2_dropout_row_pass_block_cap(dev):
    """More than 8192 * 16 row chunks at spmm_cpg = 1: the dispatch raises cpg so that the datt partials of the dropout
    row pass stay inside the workspace, as without dropout."""
    h, d = 1, 64
    key = _sweep_key(dev, 16)
    x, want = _geometry_case(key, h, d)
    try:
        _lib.tune("spmm_cpg", 1)
        _lib.clear_plan_cache()
        g = _on_device(key, str(dev))
        n_cu, _, spmm = _geometry(dev)
        C = g.n_row_chunks
        assert spmm == 1 and _cpg(C, n_cu, 16, spmm) == 1 and _grid(C, 1) > MAX_ROW_BLOCKS
        cpg = -(-C // (MAX_ROW_BLOCKS * (BLOCK // 16)))
        assert cpg >= 2 and _grid(C, cpg) <= MAX_ROW_BLOCKS, (C, cpg, _grid(C, cpg))
        got, names = _run(g.csr_args(), dev, x, P_GEO)
        assert names == FAST_NAMES, names
        _check(got, want, "block cap (1, 64)", P_GEO)
    finally:
        _lib.tune_reset()
        _lib.clear_plan_cache()


# ---- 10. memory: a condition, not a measurement ----------------------------------------------------------------------
def test_fused_gatv2_dropout_step_adds_less_than_one_edge_tensor(dev):
    """On a graph of 8 M edges at (8, 8), fused_gatv2_attention_dropout_step adds less than one (E, h) fp32 tensor to
    what was allocated; the composed gatv2_attention_dropout_step adds more than three."""
    h, d = 8, 8
    g = graphs.chung_lu_graph(20000, 8_000_000, alpha=0.5, seed=2).to(dev)
    edge_tensor = g.n_edges * h * 4
    gen = torch.Generator().manual_seed(1)
    xl, xr, dO = (torch.randn(20000, h, d, generator=gen).to(dev) for _ in range(3))
    att = (torch.randn(h, d, generator=gen) / d ** 0.5).to(dev)

    def added(step):
        peaks = []
        for _ in range(2):      # the first run also builds the plans
            leaves = [t.clone().requires_grad_(True) for t in (xl, xr, att)]
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            out = step(g, *leaves, dO, 0.6, SEED, OFFSET, SLOPE)
            torch.cuda.synchronize()
            peaks.append(torch.cuda.max_memory_allocated(dev) - base)
            del out, leaves
        return peaks[1]
    fused = added(functions.fused_gatv2_attention_dropout_step)
    composed = added(functions.gatv2_attention_dropout_step)
    print("added memory: fused %.1f MB, composed %.1f MB, one (E, h) tensor %.1f MB" % (
        fused / 2 ** 20, composed / 2 ** 20, edge_tensor / 2 ** 20))
    assert fused < edge_tensor, (fused, edge_tensor)
    assert composed > 3 * edge_tensor, (composed, edge_tensor)
