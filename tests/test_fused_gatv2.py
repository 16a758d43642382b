"""GPU tier of the fused GATv2 attention layer: graphop.gatv2_attention_forward / _backward, functions.FusedGATv2Attention
and functions.fused_gatv2_attention_step against float64 torch autograd on the CPU through
gatv2_reference.gatv2_layer(..., V=None) (tests/fused_gatv2_reference.py).

Bounds: o, stats, dxl, dxr at the project's rtol = 1e-4 / atol = 1e-5 against float64 (1e-10 / 1e-10 in fp64).  datt sums
E terms of mixed sign, so it is held to |err| <= K * S[k, c] with S = sum_e |ds[e, k] * LeakyReLU(z[e, k, c])|, ds from the
reference (with_scores=True and retain_grad()), K = 1e-6 (1e-12 in fp64).  Every measured ratio is printed.
Measured on an MI355X: datt at most 2.7e-7 * S in fp32 (the graph with rows of up to 5000 slots; 9.3e-8 * S elsewhere) and
2.4e-16 * S in fp64, so K stays at 1e-6; o, stats, dxl, dxr at most 0.33 of their bound.
Inputs: xl, xr, dO standard normal, att standard normal / sqrt(d), so the scores are O(1) at every d."""
import functools

import pytest
import torch

import fused_gatv2_reference as R
from custom_op_benchmark_amd import _lib, functions, graphop as ops, graphs
from gat_reference import reorder_chunks
from test_gat_launch_geometry import (BLOCK, MAX_ROW_BLOCKS, _assert_cpg, _cpg, _geometry, _graph, _grid, _on_device,
                                      _shifted, _shuffled, _sweep_key)
from util import random_graph

pytestmark = pytest.mark.gpu

SLOPE = 0.2
FAST_NAMES = {"gv2attn_fwd": "k_gv2attn_fwd_f32", "gv2attn_pack": "k_gv2attn_pack_f32",
              "gv2attn_bwd_row": "k_gv2attn_bwd_row_f32", "gv2attn_bwd_col": "k_gv2attn_bwd_col_f32",
              "gv2attn_datt_fin": "k_gv2attn_datt_fin_f32"}
GENERIC_NAMES = {"gv2attn_fwd": "k_gv2attn_fwd_generic", "gv2attn_pack": "k_gv2attn_pack_generic",
                 "gv2attn_bwd_row": "k_gv2attn_bwd_row_generic", "gv2attn_bwd_col": "k_gv2attn_bwd_col_generic"}
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


def _run(a8, dev, x, slope=SLOPE):
    """(o, stats, dxl, dxr, datt) through graphop.gatv2_attention_forward / _backward, and the kernels launched"""
    xl, xr, att, dO = (t.to(dev) for t in x)

    def go():
        o, stats = ops.gatv2_attention_forward(*a8[:4], xl, xr, att, slope)
        return [o, stats] + ops.gatv2_attention_backward(*a8, xl, xr, att, o, stats, dO, slope)
    return _profiled(go)


def _check(got, want, what, dtype=torch.float32):
    """got = (o, stats, dxl, dxr, datt) on the device, want = R.reference(...)"""
    tol, K = (R.TOL32, R.K32) if dtype == torch.float32 else (R.TOL64, R.K64)
    for name, x, y in zip(OUT, got, want):
        assert x.dtype == dtype and x.shape == y.shape, (what, name, x.dtype, x.shape, y.shape)
        print("%s %s: %.3f of the bound" % (what, name, R.ratio(x, y, tol)))
    r = R.datt_ratio(got[4], want[4], want[5])
    print("%s datt: max |err| / S = %.3g (bound %.1g)" % (what, r, K))
    for name, x, y in zip(OUT, got, want):
        torch.testing.assert_close(x.cpu().double(), y.double(), **tol, msg=lambda m: "%s %s: %s" % (what, name, m))
    assert got[4].dtype == dtype and got[4].shape == want[4].shape
    assert r <= K, "%s datt: max |err| / S = %g" % (what, r)


# ---- the irregular graph -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_size", [3, 32])
@pytest.mark.parametrize("d", [8, 16, 32])
@pytest.mark.parametrize("h", [1, 2, 3, 4, 8])
def test_fused_gatv2_matches_torch(dev, h, d, chunk_size):
    """A fifth of the rows empty, one hub row above the 1024-slot long-segment bound; fp32 and fp64; the fast kernels at
    (2, 32), (4, 16), (4, 32), (8, 8), (8, 16), (8, 32), the generic ones elsewhere and in fp64."""
    g = R.irregular_graph(chunk_size)
    deg = torch.bincount(g.src, minlength=g.n_src)
    assert int(deg.max()) > 1024 and 0.1 < float((deg == 0).float().mean()) < 0.3
    gd = g.to(dev)
    for dtype in (torch.float32, torch.float64):
        x = R.inputs(g, h, d, seed=h + d + chunk_size, dtype=dtype)
        got, names = _run(gd.csr_args(), dev, x)
        fast = dtype == torch.float32 and (h, d) in R.FAST
        assert names == (FAST_NAMES if fast else GENERIC_NAMES), names
        want = R.reference(g, *x, SLOPE)
        empty = deg == 0
        assert not got[0].cpu()[empty].any() and bool((got[1].cpu()[empty][..., 0] == -1e9).all())
        assert not got[1].cpu()[empty][..., 1].any()
        _check(got, want, "(%d, %d) chunk %d %s" % (h, d, chunk_size, str(dtype)[6:]), dtype)


# ---- row lengths around the batch and long-segment edges ------------------------------------------------------------
@pytest.mark.parametrize("h,d", [(1, 64), (4, 32), (8, 32)])
def test_fused_gatv2_row_lengths_at_the_batch_and_long_segment_edges(dev, h, d):
    """Rows of exactly 1, SB - 1, SB, SB + 1 (SB = 16, 8, 4 slots per batch of the forward at the three row widths),
    1024, 1025, 2049 and 5000 slots; the short part of the forward's grid ends in a partly filled workgroup."""
    g = R.edge_rows_graph()
    deg = torch.bincount(g.src, minlength=g.n_src)
    sb = 16 // (h * d // 64)
    for n in (1, sb - 1, sb, sb + 1, 1024, 1025, 2049, 5000):
        assert int((deg == n).sum()) >= 1, n
    gd = g.to(dev)
    plan = _lib.get_plan(gd.row, gd.ptr_r, gd.eid_r, gd.indices_r, g.n_dst)
    assert plan.info.row_owned and plan.info.n_segments == int((deg > 0).sum()) and plan.info.n_segments % 16 != 0
    assert plan.info.max_segment_len == 5000
    x = R.inputs(g, h, d, seed=h * 100 + d)
    got, names = _run(gd.csr_args(), dev, x)
    assert names == FAST_NAMES, names
    _check(got, R.reference(g, *x, SLOPE), "edge rows (%d, %d)" % (h, d))


# ---- slopes, ties and large scores on a rectangular graph -----------------------------------------------------------
@pytest.mark.parametrize("kind", ["ties", "large"])
@pytest.mark.parametrize("h,d", [(1, 64), (4, 16), (3, 5)])
@pytest.mark.parametrize("slope", [0.2, 0.0, -0.1, 1.0])
def test_fused_gatv2_slopes_ties_and_large_scores(dev, slope, h, d, kind):
    """ties: integer-valued xl, xr with xr = -xl on shared ids, z == 0 exactly on at least a tenth of the elements (a tie
    takes the slope).  large: |s| above 50, where an exp without the running maximum overflows."""
    g = R.slopes_graph()
    assert g.n_src != g.n_dst
    x = R.inputs(g, h, d, seed=h * 100 + d, kind=kind, slope=slope)
    want = R.reference(g, *x, slope)
    if kind == "ties":
        assert ((x[0][g.src] + x[1][g.dst]) == 0).float().mean() >= 0.1
    else:
        assert float(want[6].abs().max()) > 50
    got, names = _run(g.to(dev).csr_args(), dev, x, slope)
    assert names == (FAST_NAMES if (h, d) in R.FAST else GENERIC_NAMES), names
    _check(got, want, "slope %g %s (%d, %d)" % (slope, kind, h, d))


# ---- every fast shape: planned, NULL plan, autograd -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chung_lu():
    return graphs.chung_lu_graph(20000, 200000, alpha=0.5, seed=1)


def _c_abi(g, dev, xl, xr, att, dO, plan_r, plan_c):
    """One forward + backward through the C ABI with the given plan handles (None: plan = NULL)"""
    P, l, st = _lib.ptr, _lib.lib(), _lib.stream_of(xl)
    h, d = (1, xl.size(1)) if xl.dim() == 2 else (xl.size(1), xl.size(2))
    o, stats = torch.empty_like(xl), torch.empty((g.n_src, h, 2), device=dev)
    dxl, dxr, datt = torch.empty_like(xl), torch.empty_like(xr), torch.empty_like(att)
    ws = torch.empty(max(ops._gatv2_attention_workspace_values(g.n_src, g.n_row_chunks, h, d), 1), device=dev)
    _lib.check(l.graphop_gatv2_attention_forward(_lib.F32, P(g.row), P(g.ptr_r), P(g.eid_r), P(g.indices_r), P(xl), P(xr),
                                                 P(att), P(o), P(stats), g.n_row_chunks, g.n_edges, g.n_src, g.n_dst, h,
                                                 d, SLOPE, plan_r, st))
    _lib.check(l.graphop_gatv2_attention_backward(_lib.F32, *(P(t) for t in g.csr_args()), P(xl), P(xr), P(att), P(o),
                                                  P(stats), P(dO), P(dxl), P(dxr), P(datt), P(ws), ws.numel() * 4,
                                                  g.n_row_chunks, g.n_col_chunks, g.n_edges, g.n_src, g.n_dst, h, d,
                                                  SLOPE, plan_r, plan_c, st))
    return [o, stats, dxl, dxr, datt]


@pytest.mark.parametrize("h,d", R.FAST)
def test_fused_gatv2_every_fast_shape_planned_null_plan_and_autograd(dev, h, d):
    """The C ABI with plans launches the fast kernels, with plan = NULL the generic ones (names from the launch profile);
    both, and the FusedGATv2Attention autograd path, sit inside the bounds; two planned runs give bit-equal o, stats, datt."""
    g0 = _chung_lu()
    g = g0.to(dev)
    x = R.inputs(g0, h, d, seed=h * 100 + d)
    xl, xr, att, dO = (t.to(dev) for t in x)
    plan_r = _lib.get_plan(g.row, g.ptr_r, g.eid_r, g.indices_r, g.n_dst)
    plan_c = _lib.get_plan(g.col, g.ptr_c, g.eid_c, g.indices_c, g.n_src)
    want = R.reference(g0, *x, SLOPE)
    planned, names = _profiled(lambda: _c_abi(g, dev, xl, xr, att, dO, plan_r.handle, plan_c.handle))
    assert names == FAST_NAMES, names
    again = _c_abi(g, dev, xl, xr, att, dO, plan_r.handle, plan_c.handle)
    for i in (0, 1, 4):
        assert torch.equal(planned[i], again[i]), "run-to-run difference in %s" % (OUT + ("datt",))[i]
    unplanned, names = _profiled(lambda: _c_abi(g, dev, xl, xr, att, dO, None, None))
    assert names == GENERIC_NAMES, names
    _check(planned, want, "planned (%d, %d)" % (h, d))
    _check(unplanned, want, "NULL plan (%d, %d)" % (h, d))
    leaves = [t.clone().requires_grad_(True) for t in (xl, xr, att)]
    o = functions.fused_gatv2_attention_step(g, *leaves, dO, SLOPE)
    torch.cuda.synchronize()
    _check([o.detach(), planned[1]] + [t.grad for t in leaves], want, "autograd (%d, %d)" % (h, d))
    assert torch.equal(o.detach(), planned[0])


# ---- the backward passes at the launch geometry of large graphs ------------------------------------------------------
CAP_HD = [(1, 64), (4, 32), (8, 32)]


@functools.lru_cache(maxsize=None)
def _geometry_case(key, h, d):
    g = _graph(*key)
    x = R.inputs(g, h, d, seed=h * 100 + d + 3)
    return x, R.reference(g, *x, SLOPE)


@pytest.mark.parametrize("hd", CAP_HD)
@pytest.mark.parametrize("cpg", [2, 3, 16])
def test_fused_gatv2_backward_at_cpg(dev, cpg, hd):
    """Both backward passes with cpg in {2, 3, 16} chunks per lane group: the row-change branch, the plain store of a
    node inside a group and the clipped last group all run."""
    key = _sweep_key(dev, cpg)
    g = _on_device(key, str(dev))
    _assert_cpg(g, dev, 16, cpg)
    n_cu, _, spmm = _geometry(dev)
    assert _grid(g.n_row_chunks, _cpg(g.n_row_chunks, n_cu, 16, spmm)) <= MAX_ROW_BLOCKS     # the block cap is idle here
    for plan in (_lib.get_plan(g.row, g.ptr_r, g.eid_r, g.indices_r, g.n_dst),
                 _lib.get_plan(g.col, g.ptr_c, g.eid_c, g.indices_c, g.n_src)):
        assert plan.info.row_owned and plan.info.rows_sorted, "the plan does not own its rows: no plain stores"
    x, want = _geometry_case(key, *hd)
    got, names = _run(g.csr_args(), dev, x)
    assert names == FAST_NAMES, names
    _check(got, want, "cpg=%d %s" % (cpg, hd))


@pytest.mark.parametrize("hd", CAP_HD)
def test_fused_gatv2_backward_unordered_chunks_at_cpg(dev, hd):
    """Chunk lists in random order at cpg >= 3: the OWNED = false forms of both backward passes; the forward needs a
    row_owned plan and takes its generic form."""
    key, csr = _shuffled(dev)
    x, want = _geometry_case(key, *hd)
    got, names = _run(csr, dev, x)
    assert names == dict(FAST_NAMES, gv2attn_fwd="k_gv2attn_fwd_generic"), names
    _check(got, want, "unordered %s" % (hd,))


@pytest.mark.parametrize("hd", CAP_HD)
def test_fused_gatv2_row_pass_block_cap(dev, hd):
    """More than 8192 * 16 row chunks at spmm_cpg = 1: the row pass would launch more than 8192 workgroups; the dispatch
    raises cpg to ceil(C / (8192 * 16)) so that the datt partials stay inside the workspace."""
    key = _sweep_key(dev, 16)
    x, want = _geometry_case(key, *hd)
    try:
        _lib.tune("spmm_cpg", 1)
        _lib.clear_plan_cache()
        g = _on_device(key, str(dev))
        n_cu, _, spmm = _geometry(dev)
        C = g.n_row_chunks
        assert spmm == 1 and _cpg(C, n_cu, 16, spmm) == 1 and C > MAX_ROW_BLOCKS * 16
        assert _grid(C, 1) > MAX_ROW_BLOCKS, "the block cap is no longer reached: %d chunks give %d workgroups" % (
            C, _grid(C, 1))
        cpg = -(-C // (MAX_ROW_BLOCKS * (BLOCK // 16)))
        assert cpg >= 2 and _grid(C, cpg) <= MAX_ROW_BLOCKS, (C, cpg, _grid(C, cpg))
        h, d = hd
        assert ops._gatv2_attention_workspace_values(g.n_src, C, h, d) >= g.n_src * h * 4 + _grid(C, cpg) * h * d
        got, names = _run(g.csr_args(), dev, x)
        assert names == FAST_NAMES, names
        _check(got, want, "block cap %s" % (hd,))
    finally:
        _lib.tune_reset()
        _lib.clear_plan_cache()


# ---- fall-backs ----------------------------------------------------------------------------------------------------------
def test_fused_gatv2_misaligned_tables_fall_back(dev):
    """xl, xr or att 4 bytes off: every pass generic.  o, stats or dO 4 bytes off in the backward: its passes generic after
    a fast forward.  Same results."""
    g0 = random_graph(600, 723, 7200, seed=91, chunk_size=32, zero_rows=0.1, hub=1100)
    g = g0.to(dev)
    a8 = g.csr_args()
    x = R.inputs(g0, 4, 16, seed=5)
    want = R.reference(g0, *x, SLOPE)
    got, names = _run(a8, dev, x)
    assert names == FAST_NAMES, names
    _check(got, want, "aligned")
    for i, name in enumerate(("xl", "xr", "att")):
        t = [v.to(dev) for v in x]
        t[i] = _shifted(t[i])
        got, names = _run(a8, dev, t)
        assert names == GENERIC_NAMES, (name, names)
        _check(got, want, "%s shifted" % name)
    xl, xr, att, dO = (v.to(dev) for v in x)
    for name in ("o", "stats", "dO"):
        def go():
            o, stats = ops.gatv2_attention_forward(*a8[:4], xl, xr, att, SLOPE)
            extra = dict(o=o, stats=stats, dO=dO)
            extra[name] = _shifted(extra[name])
            return [o, stats] + ops.gatv2_attention_backward(*a8, xl, xr, att, extra["o"], extra["stats"], extra["dO"],
                                                             SLOPE)
        got, names = _profiled(go)
        assert names == dict(GENERIC_NAMES, gv2attn_fwd="k_gv2attn_fwd_f32"), (name, names)
        _check(got, want, "%s shifted" % name)


def test_fused_gatv2_shuffled_chunks_in_fp64_take_the_generic_path(dev):
    g = random_graph(250, 190, 5000, seed=11, chunk_size=8, zero_rows=0.2, hub=500)
    gen = torch.Generator().manual_seed(3)
    pr = reorder_chunks(g.ptr_r, g.row, g.eid_r, g.indices_r, torch.randperm(g.n_row_chunks, generator=gen))
    pc = reorder_chunks(g.ptr_c, g.col, g.eid_c, g.indices_c, torch.randperm(g.n_col_chunks, generator=gen))
    csr = tuple(t.to(dev) for t in (pr[1], pr[0], pr[2], pr[3], pc[1], pc[0], pc[2], pc[3]))
    assert not _lib.get_plan(*csr[:4], g.n_dst).info.row_owned
    assert not _lib.get_plan(*csr[4:], g.n_src).info.row_owned
    x = R.inputs(g, 3, 8, seed=2, dtype=torch.float64)
    got, names = _run(csr, dev, x)
    assert names == GENERIC_NAMES, names
    _check(got, R.reference(g, *x, SLOPE), "shuffled fp64 (3, 8)", torch.float64)


# ---- autograd ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,d", [(1, 3), (2, 4)])
def test_fused_gatv2_gradcheck(dev, h, d):
    g = random_graph(12, 10, 50, seed=4, chunk_size=3, hub=8).to(dev)
    gen = torch.Generator().manual_seed(0)
    xl = torch.randn(R.node_shape(g.n_src, h, d), generator=gen, dtype=torch.float64).to(dev).requires_grad_(True)
    xr = torch.randn(R.node_shape(g.n_dst, h, d), generator=gen, dtype=torch.float64).to(dev).requires_grad_(True)
    att = torch.randn(R.node_shape(1, h, d)[1:], generator=gen, dtype=torch.float64).to(dev).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b, c: functions.FusedGATv2Attention.apply(*g.csr_args(), a, b, c, SLOPE),
                                    (xl, xr, att), nondet_tol=1e-12)


def test_fused_gatv2_function_saves_no_edge_tensor(dev):
    g = random_graph(60, 50, 900, seed=8, chunk_size=8).to(dev)
    xl, xr, att, dO = (t.to(dev) for t in R.inputs(g, 4, 16, seed=1))
    xl, xr, att = (t.requires_grad_(True) for t in (xl, xr, att))
    o = functions.FusedGATv2Attention.apply(*g.csr_args(), xl, xr, att, SLOPE)
    saved = o.grad_fn.saved_tensors
    assert len(saved) == 13 and [t.data_ptr() for t in saved[8:11]] == [xl.data_ptr(), xr.data_ptr(), att.data_ptr()]
    assert all(t.size(0) != g.n_edges for t in saved[8:]) and saved[12].shape == (g.n_src, 4, 2)
    o.backward(dO)
    stats = saved[12]
    want = ops.gatv2_attention_backward(*g.csr_args(), xl.detach(), xr.detach(), att.detach(), o.detach(), stats, dO, SLOPE)
    for got, w in zip((xl.grad, xr.grad, att.grad), want):
        torch.testing.assert_close(got, w, rtol=1e-4, atol=1e-5)


# ---- bindings ------------------------------------------------------------------------------------------------------------
def test_fused_gatv2_ctypes_compiled_extension_and_torch_ops_agree(dev):
    ext = ops.cpp_ext
    if ext is None:
        pytest.skip("graphop_cpp.so not built (run __graft_entry__.build())")
    g0 = random_graph(500, 400, 8000, seed=6, chunk_size=32, hub=900)
    g = g0.to(dev)
    a8 = g.csr_args()
    for h, d in ((1, 64), (4, 16), (3, 5)):
        xl, xr, att, dO = (x.to(dev) for x in R.inputs(g0, h, d, seed=h))
        f0 = ops.gatv2_attention_forward(*a8[:4], xl, xr, att, -0.1)
        f1 = ext.gatv2_attention_forward(*a8[:4], xl, xr, att, -0.1)
        f2 = torch.ops.graphop.gatv2_attention_forward(*a8[:4], xl, xr, att, -0.1)
        assert len(f0) == len(f1) == len(f2) == 2
        for u, v, w in zip(f0, f1, f2):
            if (h, d) in R.FAST:      # the fast forward uses no atomics: one result, bit for bit
                assert torch.equal(u, v) and torch.equal(u, w)
            torch.testing.assert_close(u, v, rtol=1e-4, atol=1e-5)
            torch.testing.assert_close(u, w, rtol=1e-4, atol=1e-5)
        o, stats = f0
        b0 = ops.gatv2_attention_backward(*a8, xl, xr, att, o, stats, dO, -0.1)
        b1 = ext.gatv2_attention_backward(*a8, xl, xr, att, o, stats, dO, negative_slope=-0.1)
        b2 = torch.ops.graphop.gatv2_attention_backward(*a8, xl, xr, att, o, stats, dO, -0.1)
        assert len(b0) == len(b1) == len(b2) == 3
        for u, v, w in zip(b0, b1, b2):   # (rows split between lane groups are added by atomics: not bitwise)
            torch.testing.assert_close(u, v, rtol=1e-4, atol=1e-4)
            torch.testing.assert_close(u, w, rtol=1e-4, atol=1e-4)
    d0 = ext.gatv2_attention_forward(*a8[:4], xl, xr, att)
    d1 = ops.gatv2_attention_forward(*a8[:4], xl, xr, att)
    torch.testing.assert_close(d0[0], d1[0], rtol=1e-4, atol=1e-5)


def test_fused_gatv2_rejects_mismatched_tables(dev):
    g = random_graph(40, 40, 200, seed=1, chunk_size=8).to(dev)
    xl = torch.rand(40, 4, 8, device=dev)
    att = torch.rand(4, 8, device=dev)
    a4 = (g.row, g.ptr_r, g.eid_r, g.indices_r)
    with pytest.raises(RuntimeError, match="same h"):
        ops.gatv2_attention_forward(*a4, xl, torch.rand(40, 2, 8, device=dev), att)
    with pytest.raises(RuntimeError, match="same dtype"):
        ops.gatv2_attention_forward(*a4, xl, xl.clone(), att.double())
    with pytest.raises(RuntimeError, match="same d"):
        ops.gatv2_attention_forward(*a4, xl, torch.rand(40, 4, 16, device=dev), att)
    with pytest.raises(RuntimeError, match="same d"):
        torch.ops.graphop.gatv2_attention_forward(*a4, xl, xl.clone(), torch.rand(8, device=dev))
    o, stats = ops.gatv2_attention_forward(*a4, xl, xl.clone(), att)
    for op in (ops.gatv2_attention_backward, torch.ops.graphop.gatv2_attention_backward):
        with pytest.raises(RuntimeError, match="o must be"):
            op(*g.csr_args(), xl, xl.clone(), att, o[:, :2].contiguous(), stats, o.clone())
        with pytest.raises(RuntimeError, match="o must be"):
            op(*g.csr_args(), xl, xl.clone(), att, o, stats[:, :2].contiguous(), o.clone())
        with pytest.raises(RuntimeError, match="dO must match"):
            op(*g.csr_args(), xl, xl.clone(), att, o, stats, o[:20].contiguous())
        with pytest.raises(RuntimeError, match="same dtype"):
            op(*g.csr_args(), xl, xl.clone(), att, o, stats, o.double())


# ---- memory: a condition, not a measurement ----------------------------------------------------------------------------
def test_fused_gatv2_step_adds_less_than_one_edge_tensor(dev):
    """On a graph of 8 M edges at (8, 8), fused_gatv2_attention_step adds less than one (E, h) fp32 tensor to what was
    allocated; the composed gatv2_attention_step (V=None) adds more than two."""
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
            out = step(g, *leaves, dO, SLOPE)
            torch.cuda.synchronize()
            peaks.append(torch.cuda.max_memory_allocated(dev) - base)
            del out, leaves
        return peaks[1]
    fused, composed = added(functions.fused_gatv2_attention_step), added(functions.gatv2_attention_step)
    print("added memory: fused %.1f MB, composed %.1f MB, one (E, h) tensor %.1f MB" % (
        fused / 2 ** 20, composed / 2 ** 20, edge_tensor / 2 ** 20))
    assert fused < edge_tensor, (fused, edge_tensor)
    assert composed > 2 * edge_tensor, (composed, edge_tensor)
