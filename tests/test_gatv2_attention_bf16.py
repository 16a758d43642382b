"""GPU tier of the fused GATv2 layer on bfloat16 tables (kernels_gatv2_attn_bf16.h), with and without
attention dropout, against the plain float64 reference of gatv2_bf16_reference.py.  Bounds: o, dxl, dxr: BF_TOL of
test_attention_bf16.py (one bf16 rounding, 2**-8 relative, on top of the fp32 op's rtol 1e-4 / atol 1e-5), atol / (1 - p)
with dropout; m, 1 / l: the fp32 bound alone; datt: |err| <= K32 * S + 2**-8 |want|; rows and columns without slots 0."""
import functools
import gc

import pytest
import torch

import fused_gatv2_reference as G
import gatv2_bf16_reference as R
from custom_op_benchmark_amd import functions, graphop as ops
from dropout_reference import multipliers
from test_attention_bf16 import BF_TOL, F32, _edge_graphs
from test_fused_attention import prof_tags
from util import random_graph

pytestmark = pytest.mark.gpu

TAGS = {"gatv2_attn_bf16_" + t for t in ("fwd", "pack", "bwd_row", "bwd_col", "bwd_merge", "datt_fin")}
BF, SEED, OFFSET = torch.bfloat16, 1234567, 3
# (h, d, slots per batch of Gatv2Bf16Cfg<h, d>: forward; row and column pass): L = 8; L = 16 with NV = 1; NV = 2
SB_PAIRS = [(8, 8, (8, 4)), (4, 32, (8, 4)), (8, 32, (4, 2))]


def _bf_inputs(g, h, d, seed, **kw):
    return tuple(x.to(BF) for x in G.inputs(g, h, d, seed, **kw))


def _step(a8, inp, dev, slope, p):
    """the raw ops (the dropout entries where p > 0) -> o, stats, dxl, dxr, datt"""
    xl, xr, att, dO = (x.to(dev) for x in inp)
    if p:
        o, stats = ops.gatv2_attention_dropout_forward(*a8[:4], xl, xr, att, slope, p, SEED, OFFSET)
        return (o, stats, *ops.gatv2_attention_dropout_backward(*a8, xl, xr, att, o, stats, dO, slope, p, SEED, OFFSET))
    o, stats = ops.gatv2_attention_forward(*a8[:4], xl, xr, att, slope)
    return (o, stats, *ops.gatv2_attention_backward(*a8, xl, xr, att, o, stats, dO, slope))


def _check(g, inp, got, slope, p, what):
    (xl, xr, att, dO), h = inp, 1 if inp[0].dim() == 2 else inp[0].size(1)
    o, stats, dxl, dxr, datt = (x.cpu() for x in got)
    assert o.dtype == dxl.dtype == dxr.dtype == datt.dtype == BF and stats.dtype == torch.float32
    assert o.shape == dxl.shape == xl.shape and dxr.shape == xr.shape and datt.shape == att.shape
    r3 = lambda x, n: x.double().reshape(n, h, -1)
    xl3, xr3, att2 = r3(xl, g.n_src), r3(xr, g.n_dst), att.double().reshape(h, -1)
    mult = multipliers(g.src.numpy(), g.dst.numpy(), h, p, SEED, OFFSET) if p else None
    tol = dict(rtol=BF_TOL["rtol"], atol=BF_TOL["atol"] / (1 - p))
    o0, m0, linv0 = R.forward(g.src, g.dst, g.n_src, xl3, xr3, att2, slope, mult)
    msg = lambda name: (lambda m: "%s %s: %s" % (what, name, m))
    torch.testing.assert_close(r3(o, g.n_src), o0, **tol, msg=msg("o"))
    torch.testing.assert_close(stats[..., 0].double(), m0, **F32, msg=msg("m"))
    torch.testing.assert_close(stats[..., 1].double(), linv0, **F32, msg=msg("1/l"))
    dxl0, dxr0, datt0, S = R.backward(g.src, g.dst, xl3, xr3, att2, r3(o, g.n_src), r3(dO, g.n_src), slope, mult)
    torch.testing.assert_close(r3(dxl, g.n_src), dxl0, **tol, msg=msg("dxl"))
    torch.testing.assert_close(r3(dxr, g.n_dst), dxr0, **tol, msg=msg("dxr"))
    err = (datt.double().reshape(h, -1) - datt0).abs()
    assert bool((err <= G.K32 * S + 2 ** -8 * datt0.abs()).all()), msg("datt")(float((err / (G.K32 * S + 2 ** -8 * datt0.abs())).max()))
    live, clive = torch.bincount(g.src, minlength=g.n_src) > 0, torch.bincount(g.dst, minlength=g.n_dst) > 0
    assert not o[~live].any() and not dxl[~live].any() and not dxr[~clive].any(), what


@pytest.mark.parametrize("h,d", G.FAST)
def test_every_pair_matches_the_reference(dev, h, d):
    g = G.irregular_graph(8)
    inp = _bf_inputs(g, h, d, seed=h * 100 + d)
    a8 = tuple(x.to(dev) for x in g.csr_args())
    got = {p: _step(a8, inp, dev, 0.2, p) for p in (0.0, 0.5)}
    for p in got:
        _check(g, inp, got[p], 0.2, p, "h=%d d=%d p=%g" % (h, d, p))
        assert TAGS <= prof_tags(lambda: _step(a8, inp, dev, 0.2, p))
    assert torch.equal(got[0.0][1], got[0.5][1])          # the statistics do not see the dropout


@functools.lru_cache(maxsize=None)
def _edge_cases(name, sbs):
    if name == "rows":
        return [(G.edge_rows_graph(), "", 0.2, "normal")]
    if name == "slopes":
        return [(G.slopes_graph(), "slope %g" % s, s, "ties") for s in (-0.3, 0.0, 1.0)]
    if name == "large":
        return [(G.slopes_graph(), "", 0.2, "large")]
    return [(g, what, 0.2, "normal") for sb in (sbs if name in ("tails", "repeated") else sbs[:1])
            for g, what in _edge_graphs(name, sb)]


@pytest.mark.parametrize("name", ["rows", "tails", "one_row", "single_edge", "repeated", "empty_ends", "slopes", "large"])
@pytest.mark.parametrize("h,d,sbs", SB_PAIRS)
def test_edges_of_batches_and_records(dev, h, d, sbs, name):
    """each against the reference and bitwise the same twice"""
    for g, what, slope, kind in _edge_cases(name, sbs):
        inp = _bf_inputs(g, h, d, seed=h + d, kind=kind, slope=slope)
        a8 = tuple(x.to(dev) for x in g.csr_args())
        got = _step(a8, inp, dev, slope, 0.5)
        _check(g, inp, got, slope, 0.5, "%s h=%d d=%d %s" % (name, h, d, what))
        for x, y in zip(got, _step(a8, inp, dev, slope, 0.5)):
            assert torch.equal(x, y), (name, what)


@pytest.mark.parametrize("h,d", [(4, 16), (8, 32)])          # NV = 1 and NV = 2
def test_several_chunks_per_lane_group(dev, h, d):
    """test_gat_attention_bf16.py's construction; and the merge's fixed order: two runs agree bit for bit"""
    g = random_graph(3000, 3000, 110000, seed=17, chunk_size=1)
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    n_chunks = g.row.numel()
    cpg = min(16, max(1, n_chunks // (n_cu * 16 * 4)))
    assert cpg >= 2 and n_chunks % cpg != 0, (n_chunks, n_cu, cpg)
    row, both, inside = g.row.tolist(), 0, 0
    for c0 in range(cpg, n_chunks - cpg, cpg):
        first, last = row[c0], row[c0 + cpg - 1]
        both += first != last and first == row[c0 - 1] and last == row[c0 + cpg]
        inside += first == last and first == row[c0 - 1] and last == row[c0 + cpg]
    assert both > 0 and inside > 0
    inp = _bf_inputs(g, h, d, seed=2)
    a8 = tuple(x.to(dev) for x in g.csr_args())
    got = _step(a8, inp, dev, 0.2, 0.5)
    _check(g, inp, got, 0.2, 0.5, "cpg=%d" % cpg)
    for x, y in zip(got, _step(a8, inp, dev, 0.2, 0.5)):
        assert torch.equal(x, y)


def test_the_surface(dev):
    g = G.irregular_graph(8)
    gd = g.to(dev); a8 = gd.csr_args()
    inp = tuple(x.to(dev) for x in _bf_inputs(g, 4, 32, seed=5))
    xl, xr, att, dO = inp
    for p in (0.0, 0.5):          # ctypes, torch.ops and the compiled extension agree bit for bit
        want = _step(a8, inp, dev, 0.2, p)
        for surface in (torch.ops.graphop, ops.cpp_ext):
            if p:
                o, stats = surface.gatv2_attention_dropout_forward(*a8[:4], xl, xr, att, 0.2, p, SEED, OFFSET)
                grads = surface.gatv2_attention_dropout_backward(*a8, xl, xr, att, o, stats, dO, 0.2, p, SEED, OFFSET)
            else:
                o, stats = surface.gatv2_attention_forward(*a8[:4], xl, xr, att, 0.2)
                grads = surface.gatv2_attention_backward(*a8, xl, xr, att, o, stats, dO, 0.2)
            for x, y in zip((o, stats, *grads), want):
                assert x.dtype == y.dtype and torch.equal(x, y)
    o0, stats0 = ops.gatv2_attention_dropout_forward(*a8[:4], xl, xr, att, 0.2, 0.0, SEED, OFFSET)
    at0 = (o0, stats0, *ops.gatv2_attention_dropout_backward(*a8, xl, xr, att, o0, stats0, dO, 0.2, 0.0, SEED, OFFSET))
    for x, y in zip(at0, _step(a8, inp, dev, 0.2, 0.0)):
        assert torch.equal(x, y)
    for p in (0.0, 0.5):
        leaves = [x.clone().requires_grad_(True) for x in (xl, xr, att)]
        o = functions.fused_gatv2_attention_dropout_step(gd, *leaves, dO, p, SEED, OFFSET) if p else \
            functions.fused_gatv2_attention_step(gd, *leaves, dO)
        want = _step(a8, inp, dev, 0.2, p)
        for x, y in zip((o.detach(), *(t.grad for t in leaves)), (want[0], *want[2:])):
            assert x.dtype == BF and torch.equal(x, y)
    # unsupported: the library's message, never an upcast; the edge form and the other GATv2 ops keep refusing the dtype
    odd = [torch.zeros(s, dtype=BF, device=dev) for s in ((g.n_src, 3, 8), (g.n_dst, 3, 8), (3, 8))]
    with pytest.raises(RuntimeError, match=r"\(h, d\) = \(3, 8\) is not in the bfloat16 set"):
        ops.gatv2_attention_forward(*a8[:4], *odd)
    xe = torch.zeros((g.src.numel(), 4, 32), dtype=BF, device=dev)
    with pytest.raises(RuntimeError, match="float32 / float64"):
        ops.gatv2_attention_dropout_forward(*a8[:4], xl, xr, att, 0.2, 0.5, SEED, OFFSET, xe=xe)
    with pytest.raises(RuntimeError, match="float32 / float64"):
        ops.gatv2_scores_forward(*a8[:4], xl, xr, att)


def test_step_replays_from_a_hip_graph(dev):
    g = G.irregular_graph(8).to(dev)
    xl, xr, att, dO = (x.to(dev) for x in _bf_inputs(G.irregular_graph(8), 8, 32, seed=6))
    leaves = [x.clone().requires_grad_(True) for x in (xl, xr, att)]
    step = lambda: functions.fused_gatv2_attention_dropout_step(g, *leaves, dO, 0.5, SEED, OFFSET)
    gc.collect()          # (freeing a plan synchronises the device: nothing may be finalised during the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # plans are made here, outside the capture
        eager = step().detach().clone()
    torch.cuda.current_stream().wait_stream(side)
    want = (eager, *(t.grad.clone() for t in leaves))
    for t in leaves:
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            o = step()
    finally:
        gc.enable()
    for _ in range(2):
        for x in (o, *(t.grad for t in leaves)):
            x.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip((o, *(t.grad for t in leaves)), want):
            assert torch.equal(x.detach(), y)
