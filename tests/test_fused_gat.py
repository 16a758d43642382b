"""GPU tier of the fused GAT attention: graphop.gat_attention_forward / _backward, functions.FusedGATAttention and
functions.fused_gat_attention_step against float64 torch autograd on the CPU (tests/gat_reference.py::gat_layer) and
against the composed gat_attention_step (GATScores -> SparseSoftmax -> VectorSPMM)."""
import pytest
import torch

from custom_op_benchmark_amd import _lib, functions, graphop as ops, graphs
from gat_reference import gat_layer, reorder_chunks
from util import random_graph

pytestmark = pytest.mark.gpu

FAST_HD = [(1, 64), (2, 32), (2, 64), (4, 16), (4, 32), (4, 64), (8, 8), (8, 16), (8, 32)]


def _inputs(g, h, d, dtype, seed, ties=False, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    shape = (lambda n: (n,) if h == 1 else (n, h))
    if ties:   # small integers with el = -er on shared ids: z == 0 exactly on many edges
        el = torch.randint(-3, 4, shape(g.n_src), generator=gen).to(dtype)
        er = torch.randint(-3, 4, shape(g.n_dst), generator=gen).to(dtype)
        m = min(g.n_src, g.n_dst)
        er[:m] = -el[:m]
    else:
        el = torch.randn(shape(g.n_src), generator=gen, dtype=dtype) * scale
        er = torch.randn(shape(g.n_dst), generator=gen, dtype=dtype) * scale
    vs = (lambda n: (n, d) if h == 1 else (n, h, d))
    V = torch.randn(vs(g.n_dst), generator=gen, dtype=dtype)
    dO = torch.randn(vs(g.n_src), generator=gen, dtype=dtype)
    return el, er, V, dO


def _reference(g, el, er, V, dO, s):
    r = [x.double().requires_grad_(True) for x in (el, er, V)]
    o = gat_layer(g.src, g.dst, g.n_src, r[0], r[1], r[2], s)
    o.backward(dO.double())
    return o.detach(), r[0].grad, r[1].grad, r[2].grad


def _fused(a8, dev, el, er, V, dO, s):
    eld, erd, Vd = (x.to(dev) for x in (el, er, V))
    o, stats = ops.gat_attention_forward(*a8[:4], eld, erd, Vd, s)
    grads = ops.gat_attention_backward(*a8, eld, erd, Vd, o, stats, dO.to(dev), s)
    torch.cuda.synchronize()
    return [o] + grads


def _compare(got, want, dtype, what=""):
    tol = dict(rtol=1e-4, atol=1e-5) if dtype == torch.float32 else dict(rtol=1e-10, atol=1e-10)
    for name, x, y in zip(("o", "del", "der", "dV"), got, want):
        assert x.dtype == dtype and x.shape == y.shape, (name, x.shape, y.shape)
        torch.testing.assert_close(x.cpu().double(), y, **tol, msg=lambda m: "%s%s: %s" % (what, name, m))


@pytest.mark.parametrize("chunk_size", [3, 32])
def test_fused_gat_matches_the_float64_reference(dev, chunk_size):
    """A fifth of the rows empty and one hub row above the long-segment bound (1024 slots): h in {1, 2, 3, 4, 8} x
    d in {8, 16, 32}, fp32 and fp64 (the (h, d) pairs of the fast set run the fast kernels in fp32)."""
    g = random_graph(300, 300, 3000, seed=chunk_size, chunk_size=chunk_size, zero_rows=0.2, hub=1500)
    gd = g.to(dev)
    a8 = gd.csr_args()
    for h in (1, 2, 3, 4, 8):
        for d in (8, 16, 32):
            el, er, V, dO = _inputs(g, h, d, torch.float64, seed=h * 100 + d)
            want = _reference(g, el, er, V, dO, 0.2)
            for dtype in (torch.float32, torch.float64):
                got = _fused(a8, dev, *(x.to(dtype) for x in (el, er, V, dO)), 0.2)
                _compare(got, want, dtype, "h=%d d=%d %s " % (h, d, dtype))


@pytest.mark.parametrize("slope", [0.2, 0.0, -0.1, 1.0])
def test_fused_gat_slopes_ties_and_large_scores(dev, slope):
    """Fast (8, 16) and generic (3, 8) shapes: z == 0 on many edges (the tie takes the slope), and |z| ~ 50, where an
    exp without the row maximum would overflow fp32."""
    g = random_graph(200, 200, 4000, seed=7, chunk_size=8, zero_rows=0.1, hub=300)
    gd = g.to(dev)
    for h, d in ((8, 16), (3, 8)):
        for kind in ("ties", "large"):
            el, er, V, dO = _inputs(g, h, d, torch.float32, seed=5, ties=kind == "ties", scale=25.0)
            if kind == "ties":
                assert ((el[g.src] + er[g.dst]) == 0).float().mean() > 0.1
            else:
                assert (el[g.src] + er[g.dst]).abs().max() > 50
            _compare(_fused(gd.csr_args(), dev, el, er, V, dO, slope), _reference(g, el, er, V, dO, slope),
                     torch.float32, "%s h=%d " % (kind, h))


def test_fused_gat_fast_path_matches_the_composed_step_and_the_generic_kernels(dev):
    """Every fast (h, d) on a 20k-node Chung-Lu graph, fp32: the fused step against gat_attention_step, and the C ABI
    with plans (fast kernels) against plan = NULL (generic kernels); kernel names from the launch profile."""
    g = graphs.chung_lu_graph(20000, 200000, alpha=0.5, seed=3).to(dev)
    a8 = g.csr_args()
    plan_r = _lib.get_plan(g.row, g.ptr_r, g.eid_r, g.indices_r, g.n_dst)
    plan_c = _lib.get_plan(g.col, g.ptr_c, g.eid_c, g.indices_c, g.n_src)
    P, l, F32 = _lib.ptr, _lib.lib(), _lib.F32
    tags = ("gat_attn_stats", "gat_attn_fwd", "gat_attn_pack", "gat_attn_bwd_row", "gat_attn_bwd_col")
    for h, d in FAST_HD:
        el, er, V, dO = (x.to(dev) for x in _inputs(g, h, d, torch.float32, seed=h + d))
        # the composed step
        leaves = [x.clone().requires_grad_(True) for x in (el, er, V)]
        _, _, o_ref = functions.gat_attention_step(g, *leaves, dO)
        want = [o_ref.detach()] + [x.grad for x in leaves]
        # the fused step (autograd class)
        leaves2 = [x.clone().requires_grad_(True) for x in (el, er, V)]
        o = functions.fused_gat_attention_step(g, *leaves2, dO)
        got = [o.detach()] + [x.grad for x in leaves2]
        torch.cuda.synchronize()
        for name, x, y in zip(("o", "del", "der", "dV"), got, want):
            torch.testing.assert_close(x, y, rtol=1e-4, atol=1e-5, msg=lambda m: "(%d, %d) %s: %s" % (h, d, name, m))
        # the C ABI with and without plans
        out, names = {}, {}
        _lib.profile_enable(True)
        try:
            for planned in (True, False):
                hr, hc = (plan_r.handle, plan_c.handle) if planned else (None, None)
                o2, stats = torch.empty_like(o), torch.empty((g.n_src, h, 2), device=dev)
                _lib.check(l.graphop_gat_attention_forward(F32, *(P(t) for t in a8[:4]), P(el), P(er), P(V), P(o2),
                                                           P(stats), g.n_row_chunks, g.n_edges, g.n_src, g.n_dst, h, d,
                                                           0.2, hr, _lib.stream_of(el)))
                prof = _lib.profile_read()
                kf = (prof["gat_attn_stats"]["kernel"], prof["gat_attn_fwd"]["kernel"])
                d_el, d_er, dV = torch.empty_like(el), torch.empty_like(er), torch.empty_like(V)
                ws = torch.empty(g.n_src * h * 4, device=dev)
                _lib.check(l.graphop_gat_attention_backward(
                    F32, *(P(t) for t in a8), P(el), P(er), P(V), P(o2), P(stats), P(dO), P(d_el), P(d_er), P(dV),
                    P(ws), ws.numel() * 4, g.n_row_chunks, g.n_col_chunks, g.n_edges, g.n_src, g.n_dst, h, d, 0.2, hr,
                    hc, _lib.stream_of(el)))
                prof = _lib.profile_read()
                names[planned] = kf + tuple(prof[t]["kernel"] for t in tags[2:])
                out[planned] = (o2, d_el, d_er, dV)
        finally:
            _lib.profile_enable(False)
        assert names[True] == ("k_gat_attn_stats_f32", "k_gat_attn_fwd_f32", "k_gat_attn_pack_f32",
                               "k_gat_attn_bwd_row_f32", "k_gat_attn_bwd_col_f32"), names[True]
        assert names[False] == tuple("k_%s_generic" % t for t in tags), names[False]
        for x, y, z in zip(out[True], out[False], got):
            torch.testing.assert_close(x, y, rtol=1e-4, atol=1e-5)
            torch.testing.assert_close(x, z, rtol=1e-4, atol=1e-5)


def test_fused_gat_generic_path_shuffled_chunks_rectangular_fp64(dev):
    """Chunks in random order on both orientations (row[] unsorted: no row_owned plan), fp64, h = 3, n_src != n_dst:
    o has n_src rows."""
    g = random_graph(260, 190, 5000, seed=11, chunk_size=8, zero_rows=0.2, hub=500)
    gen = torch.Generator().manual_seed(1)
    pr = reorder_chunks(g.ptr_r, g.row, g.eid_r, g.indices_r, torch.randperm(g.n_row_chunks, generator=gen))
    pc = reorder_chunks(g.ptr_c, g.col, g.eid_c, g.indices_c, torch.randperm(g.n_col_chunks, generator=gen))
    csr = tuple(t.to(dev) for t in (pr[1], pr[0], pr[2], pr[3], pc[1], pc[0], pc[2], pc[3]))
    assert not _lib.get_plan(*csr[:4], g.n_dst).info.row_owned
    for h, d, dtype in ((3, 8, torch.float64), (4, 16, torch.float32)):
        el, er, V, dO = _inputs(g, h, d, dtype, seed=h)
        got = _fused(csr, dev, el, er, V, dO, 0.2)
        assert got[0].shape == (g.n_src, h, d) and g.n_src != g.n_dst
        _compare(got, _reference(g, el, er, V, dO, 0.2), dtype, "h=%d " % h)


def test_fused_gat_gradcheck(dev):
    g = random_graph(12, 10, 50, seed=4, chunk_size=3, hub=8).to(dev)
    for h, d in ((1, 3), (2, 4)):
        el, er, V, _ = (x.to(dev) for x in _inputs(g, h, d, torch.float64, seed=h))
        inputs = tuple(x.requires_grad_(True) for x in (el, er, V))
        assert torch.autograd.gradcheck(
            lambda a, b, v: functions.FusedGATAttention.apply(*g.csr_args(), a, b, v, 0.2), inputs,
            nondet_tol=1e-12)   # (split rows are summed by float atomics: the order of the adds may differ)


def test_fused_gat_bindings_agree(dev):
    ext = ops.cpp_ext
    if ext is None:
        pytest.skip("graphop_cpp.so not built (run __graft_entry__.build())")
    g = random_graph(500, 400, 8000, seed=6, chunk_size=32, hub=900).to(dev)
    a8 = g.csr_args()
    for h, d in ((1, 64), (4, 16), (3, 8)):
        el, er, V, dO = (x.to(dev) for x in _inputs(g, h, d, torch.float32, seed=h))
        f0 = ops.gat_attention_forward(*a8[:4], el, er, V, -0.1)
        f1 = ext.gat_attention_forward(*a8[:4], el, er, V, -0.1)
        f2 = torch.ops.graphop.gat_attention_forward(*a8[:4], el, er, V, -0.1)
        for u, v, w in zip(f0, f1, f2):   # (rows split over lane groups are summed by atomics, in any order)
            torch.testing.assert_close(u, v, rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(u, w, rtol=1e-5, atol=1e-6)
        b0 = ops.gat_attention_backward(*a8, el, er, V, *f0, dO, -0.1)
        b1 = ext.gat_attention_backward(*a8, el, er, V, *f0, dO, negative_slope=-0.1)
        b2 = torch.ops.graphop.gat_attention_backward(*a8, el, er, V, *f0, dO, -0.1)
        for u, v, w in zip(b0, b1, b2):
            torch.testing.assert_close(u, v, rtol=1e-4, atol=1e-5)
            torch.testing.assert_close(u, w, rtol=1e-4, atol=1e-5)
    with pytest.raises(RuntimeError, match="V must be"):
        ops.gat_attention_forward(*a8[:4], el, er, V[:, :2])
    with pytest.raises(RuntimeError, match="dO must match"):
        ops.gat_attention_backward(*a8, el, er, V, *f0, dO[:10])


def test_fused_gat_keeps_no_edge_sized_tensor(dev):
    """h = 8, d = 8 on 8 M edges: one (E, h) fp32 tensor is 256 MB.  The fused fwd+bwd adds less than one of them to
    what is allocated before it; the composed step adds more than two."""
    g = graphs.chung_lu_graph(20000, 8_000_000, alpha=0.5, seed=0, device=dev)
    h, d = 8, 8
    one = g.n_edges * h * 4
    el, er, V, dO = (x.to(dev) for x in _inputs(g, h, d, torch.float32, seed=1))

    def peak(step):
        leaves = [x.clone().requires_grad_(True) for x in (el, er, V)]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = step(g, *leaves, dO)
        torch.cuda.synchronize()
        p = torch.cuda.max_memory_allocated() - base
        del out, leaves
        return p

    peak(functions.fused_gat_attention_step)     # plans of both orientations are built (and cached) here
    fused = peak(functions.fused_gat_attention_step)
    composed = peak(functions.gat_attention_step)
    assert fused < one, (fused, one)
    assert composed > 2 * one, (composed, one)
