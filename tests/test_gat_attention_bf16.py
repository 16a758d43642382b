"""GPU tier of the fused GAT layer on bfloat16 tables (kernels_gat_attn_bf16.h), with and without attention
dropout, against the plain float64 reference of gat_bf16_reference.py.

Tolerances: a bf16 output is the round-to-nearest of an fp32 value, half an ulp of an 8-bit significand = 2**-8 relative,
on top of the fp32 op's own bound (test_fused_gat._compare: rtol 1e-4, atol 1e-5): BF_TOL of test_attention_bf16.py.
stats are fp32 and get the fp32 bound alone -- and are bit for bit the fp32 op's on the widened el / er."""
import functools
import gc

import pytest
import torch

import gat_bf16_reference as R
from custom_op_benchmark_amd import functions, graphop as ops
from dropout_reference import multipliers
from test_attention_bf16 import BF_TOL, F32, _edge_graphs
from test_fused_attention import prof_tags
from test_fused_gat import FAST_HD, _inputs
from util import random_graph

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
TAGS = {"gat_attn_bf16_" + t for t in ("stats", "fwd", "fwd_merge", "pack", "bwd_row", "bwd_col", "bwd_merge")}
SEED, OFFSET = 1234567, 3


@functools.lru_cache(maxsize=None)
def _graph():
    """the family's graph: empty rows, a hub over many chunks, ragged last batches, n_src != n_dst"""
    return random_graph(300, 337, 2700, seed=3, chunk_size=8, zero_rows=0.2, hub=150)


def _bf_inputs(g, h, d, seed, **kw):
    return tuple(x.to(BF) for x in _inputs(g, h, d, torch.float32, seed, **kw))


def _step(a8, inp, dev, slope, p):
    """the raw ops (the dropout entries where p > 0) -> o, stats, del, der, dV"""
    el, er, V, dO = (x.to(dev) for x in inp)
    if p:
        o, stats = ops.gat_attention_dropout_forward(*a8[:4], el, er, V, slope, p, SEED, OFFSET)
        return (o, stats, *ops.gat_attention_dropout_backward(*a8, el, er, V, o, stats, dO, slope, p, SEED, OFFSET))
    o, stats = ops.gat_attention_forward(*a8[:4], el, er, V, slope)
    return (o, stats, *ops.gat_attention_backward(*a8, el, er, V, o, stats, dO, slope))


def _check(g, inp, got, slope, p, what):
    el, er, V, dO = inp
    h = 1 if el.dim() == 1 else el.size(1)
    o, stats, d_el, d_er, dV = (x.cpu() for x in got)
    assert o.dtype == d_el.dtype == d_er.dtype == dV.dtype == BF and stats.dtype == torch.float32
    assert o.shape == dO.shape and d_el.shape == el.shape and d_er.shape == er.shape and dV.shape == V.shape
    r3 = lambda x, n: x.double().reshape(n, h, -1)
    el2, er2 = el.double().reshape(g.n_src, h), er.double().reshape(g.n_dst, h)
    mult = multipliers(g.src.numpy(), g.dst.numpy(), h, p, SEED, OFFSET) if p else None
    o0, m0, linv0 = R.forward(g.src, g.dst, g.n_src, el2, er2, r3(V, g.n_dst), slope, mult)
    msg = lambda name: (lambda m: "%s %s: %s" % (what, name, m))
    torch.testing.assert_close(r3(o, g.n_src), o0, **BF_TOL, msg=msg("o"))
    torch.testing.assert_close(stats[..., 0].double(), m0, **F32, msg=msg("m"))
    torch.testing.assert_close(stats[..., 1].double(), linv0, **F32, msg=msg("1/l"))
    want = R.backward(g.src, g.dst, el2, er2, r3(V, g.n_dst), r3(o, g.n_src), r3(dO, g.n_src), slope, mult)
    for name, x, x0 in zip(("del", "der", "dV"), (d_el, d_er, dV), want):
        torch.testing.assert_close(x.double().reshape(x0.shape), x0, **BF_TOL, msg=msg(name))
    live, clive = torch.bincount(g.src, minlength=g.n_src) > 0, torch.bincount(g.dst, minlength=g.n_dst) > 0
    assert not o[~live].any() and not d_el[~live].any() and not d_er[~clive].any() and not dV[~clive].any(), what


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("h,d", FAST_HD)
def test_every_pair_matches_the_reference(dev, h, d, p):
    g = _graph()
    assert (torch.bincount(g.src, minlength=g.n_src) == 0).any()          # (slotless columns: the empty_ends case below)
    inp = _bf_inputs(g, h, d, seed=h * 100 + d)
    a8 = tuple(x.to(dev) for x in g.csr_args())
    got = _step(a8, inp, dev, 0.2, p)
    _check(g, inp, got, 0.2, p, "h=%d d=%d p=%g" % (h, d, p))
    # the statistics are the fp32 op's on the widened inputs, bit for bit
    stats32 = ops.gat_attention_forward(*a8[:4], *(x.to(dev).float() for x in inp[:3]), 0.2)[1]
    assert torch.equal(got[1], stats32)
    assert TAGS <= prof_tags(lambda: _step(a8, inp, dev, 0.2, p))


@pytest.mark.parametrize("h,d", [(4, 16), (8, 32)])          # NV = 1 and NV = 2
def test_several_chunks_per_lane_group(dev, h, d):
    """test_attention_bf16.py's construction: cpg >= 2, a short last run, groups wholly inside a row and groups that
    share both ends; and the merge's fixed order: two runs agree bit for bit"""
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


# ---- edges of the batch loop and of the record / merge scheme ---------------------------------------------------------------
# (h, d, the slots per batch of GatBf16Cfg<h, d>: forward, backward): L = 8; L = 16 with NV = 1; NV = 2
SB_PAIRS = [(8, 8, (8,)), (4, 32, (16, 8)), (8, 32, (8, 4))]


@pytest.mark.parametrize("name", ["tails", "one_row", "single_edge", "repeated", "empty_ends", "slopes"])
@pytest.mark.parametrize("h,d,sbs", SB_PAIRS)
def test_edges_of_batches_and_records(dev, h, d, sbs, name):
    """rows of 1, SB - 1, SB, SB + 1, 2 SB + 1 slots at chunk sizes 1, SB, SB + 1; one row over 600 one-slot chunks; a single
    edge; repeated (i, j) pairs; empty first and last rows and columns; negative and zero slopes on ties (z == 0)"""
    if name == "slopes":
        cases = [(_graph(), "slope %g" % s, s, True) for s in (-0.3, 0.0, 1.0)]
    else:
        cases = [(g, what, 0.2, False) for sb in (sbs if name in ("tails", "repeated") else sbs[:1])
                 for g, what in _edge_graphs(name, sb)]
    for g, what, slope, ties in cases:
        if name == "empty_ends":
            deg, cdeg = torch.bincount(g.src, minlength=g.n_src), torch.bincount(g.dst, minlength=g.n_dst)
            assert deg[0] == deg[-1] == cdeg[0] == cdeg[-1] == 0 and deg[1] == 200 and deg[-2] == 230
        inp = _bf_inputs(g, h, d, seed=h + d, ties=ties)
        a8 = tuple(x.to(dev) for x in g.csr_args())
        got = _step(a8, inp, dev, slope, 0.5)
        _check(g, inp, got, slope, 0.5, "%s h=%d d=%d %s" % (name, h, d, what))
        for x, y in zip(got, _step(a8, inp, dev, slope, 0.5)):
            assert torch.equal(x, y), (name, what)


def test_the_surface(dev):
    g = _graph()
    gd = g.to(dev)
    a8 = gd.csr_args()
    inp = tuple(x.to(dev) for x in _bf_inputs(g, 4, 32, seed=5))
    el, er, V, dO = inp
    for p in (0.0, 0.5):          # ctypes, torch.ops and the compiled extension agree bit for bit
        want = _step(a8, inp, dev, 0.2, p)
        for surface in (torch.ops.graphop, ops.cpp_ext):
            if p:
                o, stats = surface.gat_attention_dropout_forward(*a8[:4], el, er, V, 0.2, p, SEED, OFFSET)
                grads = surface.gat_attention_dropout_backward(*a8, el, er, V, o, stats, dO, 0.2, p, SEED, OFFSET)
            else:
                o, stats = surface.gat_attention_forward(*a8[:4], el, er, V, 0.2)
                grads = surface.gat_attention_backward(*a8, el, er, V, o, stats, dO, 0.2)
            for x, y in zip((o, stats, *grads), want):
                assert x.dtype == y.dtype and torch.equal(x, y)
    # the dropout entry at p = 0 is the plain entry
    o0, stats0 = ops.gat_attention_dropout_forward(*a8[:4], el, er, V, 0.2, 0.0, SEED, OFFSET)
    plain = _step(a8, inp, dev, 0.2, 0.0)
    for x, y in zip((o0, stats0, *ops.gat_attention_dropout_backward(*a8, el, er, V, o0, stats0, dO, 0.2, 0.0, SEED, OFFSET)),
                    plain):
        assert torch.equal(x, y)
    # the two Function classes on bf16 leaves
    for p in (0.0, 0.5):
        leaves = [x.clone().requires_grad_(True) for x in (el, er, V)]
        o = functions.fused_gat_attention_dropout_step(gd, *leaves, dO, p, SEED, OFFSET) if p else \
            functions.fused_gat_attention_step(gd, *leaves, dO)
        want = _step(a8, inp, dev, 0.2, p)
        for x, y in zip((o.detach(), *(t.grad for t in leaves)), (want[0], *want[2:])):
            assert x.dtype == BF and torch.equal(x, y)
    # unsupported: the library's message, never an upcast; the other GAT ops keep refusing the dtype
    odd = [torch.zeros(s, dtype=BF, device=dev) for s in ((g.n_src, 3), (g.n_dst, 3), (g.n_dst, 3, 8))]
    with pytest.raises(RuntimeError, match=r"\(h, d\) = \(3, 8\) is not in the bfloat16 set"):
        ops.gat_attention_forward(*a8[:4], *odd)
    with pytest.raises(RuntimeError, match="float32 / float64"):
        ops.gat_scores_forward(*a8[:4], el, er)


def test_step_replays_from_a_hip_graph(dev):
    g = _graph().to(dev)
    el, er, V, dO = (x.to(dev) for x in _bf_inputs(g, 8, 32, seed=6))
    leaves = [x.clone().requires_grad_(True) for x in (el, er, V)]
    step = lambda: functions.fused_gat_attention_dropout_step(g, *leaves, dO, 0.5, SEED, OFFSET)
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
