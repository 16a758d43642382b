"""GPU tier of the fused attention step on bfloat16 tables (kernels_attn_bf16.h) against the plain float64
reference of attention_bf16_reference.py.

Tolerances: a bf16 output is the round-to-nearest of an fp32 value.  bfloat16 has an 8-bit significand, so half an ulp is
up to 2**-8 relative: BF_TOL is that ONE rounding plus TOL of test_fused_attention.py for the fp32 arithmetic underneath.
It is tight -- torch's own fp32 evaluation of the reference, rounded once, uses 0.96 to 0.98 of it
(test_attention_bf16_fuzz_host.py).  stats are fp32 and get TOL alone."""
import functools
import gc

import pytest
import torch

import attention_bf16_reference as R
from custom_op_benchmark_amd import functions, graphop as ops, graphs
from test_fused_attention import TOL, prof_tags, shuffled_chunk_arrays
from util import random_graph

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, TOL[torch.float32]
BF_TOL = dict(rtol=2 ** -8 + F32["rtol"], atol=F32["atol"])
HD = [(1, 64), (1, 128), (2, 32), (2, 64), (4, 16), (4, 32), (4, 64), (8, 8), (8, 16), (8, 32), (8, 64)]
TAGS = {"attn_bf16_fwd_rows", "attn_bf16_fwd_merge", "attn_bf16_pack", "attn_bf16_rows_row", "attn_bf16_rows_col",
        "attn_bf16_bwd_merge"}


@functools.lru_cache(maxsize=None)
def _graph():
    """the family's graph: empty rows, a hub over many chunks, ragged last batches, n_q != n_k"""
    return random_graph(300, 337, 2700, seed=3, chunk_size=8, zero_rows=0.2, hub=150)


def _inputs(g, h, d, seed):
    gen = torch.Generator().manual_seed(seed)
    return tuple((torch.randn(n, h, d, generator=gen) / d ** 0.5).to(BF) for n in (g.n_src, g.n_dst, g.n_dst, g.n_src))


def _step(a8, inp, dev):
    """the raw ops -> o, stats, dQ, dK, dV"""
    Q, K, V, dO = (x.to(dev) for x in inp)
    o, stats = ops.attention_forward(*a8[:4], Q, K, V)
    return (o, stats, *ops.attention_backward(*a8, Q, K, V, o, stats, dO))


def _check(g, inp, got, what):
    Q, K, V, dO = inp
    o, stats, dQ, dK, dV = (x.cpu() for x in got)
    assert o.dtype == dQ.dtype == dK.dtype == dV.dtype == BF and stats.dtype == torch.float32
    o0, m0, linv0, _ = R.forward(g.src, g.dst, g.n_src, Q, K, V)
    live = torch.bincount(g.src, minlength=g.n_src) > 0
    torch.testing.assert_close(o.double(), o0, **BF_TOL, msg=lambda m: what + " o: " + m)
    torch.testing.assert_close(stats[live, :, 0].double(), m0[live], **F32, msg=lambda m: what + " m: " + m)
    torch.testing.assert_close(stats[..., 1].double(), linv0, **F32, msg=lambda m: what + " 1/l: " + m)
    assert not o[~live].any() and not stats[~live][..., 1].any()
    for name, x, x0 in zip(("dQ", "dK", "dV"), (dQ, dK, dV), R.backward(g.src, g.dst, Q, K, V, o, dO)):
        torch.testing.assert_close(x.double(), x0, **BF_TOL, msg=lambda m: "%s %s: %s" % (what, name, m))


@pytest.mark.parametrize("h,d", HD)
def test_every_pair_matches_the_reference(dev, h, d):
    g = _graph()
    inp = _inputs(g, h, d, seed=h * 100 + d)
    a8 = tuple(x.to(dev) for x in g.csr_args())
    _check(g, inp, _step(a8, inp, dev), "h=%d d=%d" % (h, d))
    assert TAGS <= prof_tags(lambda: _step(a8, inp, dev))


def test_several_chunks_per_lane_group(dev):
    """test_several_chunks_per_lane_group of test_attention_heads.py: cpg >= 2, a short last run, groups wholly inside a
    row and groups that share both ends; and the merge's fixed order: two runs agree bit for bit"""
    h, d = 4, 16
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
    inp = _inputs(g, h, d, seed=2)
    a8 = tuple(x.to(dev) for x in g.csr_args())
    got = _step(a8, inp, dev)
    _check(g, inp, got, "cpg=%d" % cpg)
    for x, y in zip(got, _step(a8, inp, dev)):
        assert torch.equal(x, y)


# ---- edges of the batch loop and of the record / merge scheme, one pair per SB -------------------------------------------
SB_PAIRS = [(4, 16, 8), (4, 32, 8), (4, 64, 4), (8, 64, 2)]          # (h, d, AttnBf16Cfg<h, d>::SB)


def _rows_graph(rows, n_q, n_k, chunk_size):
    """the graph whose row i holds the neighbour list rows[i] (repeats kept)"""
    src = torch.tensor([i for i, js in rows.items() for _ in js], dtype=torch.int64)
    dst = torch.tensor([j for js in rows.values() for j in js], dtype=torch.int64)
    return graphs.graph_from_coo(src, dst, n_q, n_k, chunk_size)


def _spread_inputs(g, h, d, seed):
    """Q ~ 8 randn / sqrt(d), K, V ~ randn, dO ~ randn / (4 sqrt(d)): scores of spread 8, so the running maximum moves and
    a wrong rescale or combine is a gross error (the wide8 recipe of attention_bf16_fuzz.py)"""
    gen = torch.Generator().manual_seed(seed)
    Q, K, V, dO = (torch.randn(n, h, d, generator=gen) for n in (g.n_src, g.n_dst, g.n_dst, g.n_src))
    return (Q * 8 / d ** 0.5).to(BF), K.to(BF), V.to(BF), (dO / (4 * d ** 0.5)).to(BF)


def _tails(sb):
    """rows of 1, SB - 1, SB, SB + 1 and 2 SB + 1 slots over 40 neighbours, each ending at neighbour 39: slots are stored
    by ascending neighbour id, so every row's last batch -- short in all but the row of SB slots -- re-reads the table's
    last row for the slots it does not have"""
    gen = torch.Generator().manual_seed(sb)
    return {i: torch.randperm(39, generator=gen)[:n - 1].tolist() + [39]
            for i, n in enumerate((1, max(sb - 1, 1), sb, sb + 1, 2 * sb + 1))}, 5, 40


def _edge_graphs(name, sb):
    """[(graph, what)] of one edge shape"""
    gen = torch.Generator().manual_seed(len(name))
    rnd = lambda n, n_k: torch.randint(0, n_k, (n,), generator=gen).tolist()
    if name == "tails":
        rows, n_q, n_k = _tails(sb)
        return [(_rows_graph(rows, n_q, n_k, cs), "chunk_size %d" % cs) for cs in (1, sb, sb + 1)]
    if name == "one_row":          # 600 chunks of one slot, one lane group each: every interior record has neither flag
        return [(_rows_graph({1: rnd(600, 50)}, 3, 50, 1), "")]
    if name == "two_rows":
        return [(_rows_graph({0: rnd(7, 9), 1: rnd(13, 9)}, 2, 9, cs), "chunk_size %d" % cs) for cs in (1, 8)]
    if name == "single_edge":
        return [(_rows_graph({1: [2]}, 3, 4, 8), "")]
    if name == "repeated":
        return [(_rows_graph({0: [3] * 5 + [1, 6], 2: [6] * (2 * sb + 1), 3: [0, 0, 7, 7]}, 4, 8, cs), "chunk_size %d" % cs)
                for cs in (1, 3)]
    assert name == "empty_ends"          # rows 0 and n - 1 empty, rows 1 and n - 2 hubs; columns 0 and n_k - 1 empty too
    rows = {1: [1 + j for j in rnd(200, 30)], 10: [1 + j for j in rnd(230, 30)]}
    rows.update({i: [1 + j for j in rnd(1 + i % 4, 30)] for i in (3, 4, 6, 7, 9)})
    return [(_rows_graph(rows, 12, 32, cs), "chunk_size %d" % cs) for cs in (1, 3)]


@pytest.mark.parametrize("name", ["tails", "one_row", "two_rows", "single_edge", "repeated", "empty_ends"])
@pytest.mark.parametrize("h,d,sb", SB_PAIRS)
def test_edges_of_batches_and_records(dev, h, d, sb, name):
    """against the reference, and bitwise the same twice"""
    for g, what in _edge_graphs(name, sb):
        if name == "empty_ends":
            deg, cdeg = torch.bincount(g.src, minlength=g.n_src), torch.bincount(g.dst, minlength=g.n_dst)
            assert deg[0] == deg[-1] == cdeg[0] == cdeg[-1] == 0 and deg[1] == 200 and deg[-2] == 230
        inp = _spread_inputs(g, h, d, seed=h + d)
        a8 = tuple(x.to(dev) for x in g.csr_args())
        got = _step(a8, inp, dev)
        _check(g, inp, got, "%s h=%d d=%d %s" % (name, h, d, what))
        for x, y in zip(got, _step(a8, inp, dev)):
            assert torch.equal(x, y), (name, what)


def test_the_surface(dev):
    g = _graph()
    gd = g.to(dev)
    Q, K, V, dO = (x.to(dev) for x in _inputs(g, 4, 32, seed=5))
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
    o = functions.FusedAttention.apply(*gd.csr_args(), q, k, v)
    o.backward(dO)
    q2, k2, v2 = (x.clone().requires_grad_(True) for x in (Q, K, V))
    o2 = functions.fused_attention_step(gd, q2, k2, v2, dO)
    assert o.dtype == q.grad.dtype == k.grad.dtype == v.grad.dtype == BF
    for x, y in ((o, o2), (q.grad, q2.grad), (k.grad, k2.grad), (v.grad, v2.grad)):
        assert torch.equal(x.detach(), y.detach())
    # the compiled binding answers like the ctypes one
    o3, stats3 = torch.ops.graphop.attention_forward(*gd.csr_args()[:4], Q, K, V)
    assert torch.equal(o3, o.detach()) and stats3.dtype == torch.float32
    for x, y in zip(torch.ops.graphop.attention_backward(*gd.csr_args(), Q, K, V, o3, stats3, dO), (q.grad, k.grad, v.grad)):
        assert torch.equal(x, y)
    assert ops.attention_backward_is_fused(*gd.csr_args(), Q, K) is True
    # unsupported: an error that names the condition, never an upcast
    odd = [torch.zeros(n, 3, 8, dtype=BF, device=dev).requires_grad_(True) for n in (g.n_src, g.n_dst, g.n_dst)]
    assert ops.attention_backward_is_fused(*gd.csr_args(), odd[0], odd[1]) is False
    with pytest.raises(RuntimeError, match=r"\(h, d\) = \(3, 8\) is not in the bfloat16 set"):
        functions.FusedAttention.apply(*gd.csr_args(), *odd)
    shuffled = tuple(x.to(dev) for x in shuffled_chunk_arrays(g, seed=11))
    assert ops.attention_backward_is_fused(*shuffled, Q, K) is False
    with pytest.raises(RuntimeError, match="not row_owned"):
        functions.FusedAttention.apply(*shuffled, q, k, v)
    with pytest.raises(RuntimeError, match="float32 / float64"):
        ops.attention_bias_forward(*gd.csr_args()[:4], Q, K, V, torch.zeros(g.n_edges, 4, dtype=BF, device=dev))


def test_step_replays_from_a_hip_graph(dev):
    g = _graph().to(dev)
    Q, K, V, dO = (x.to(dev) for x in _inputs(g, 8, 32, seed=6))
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
    gc.collect()          # (freeing a plan synchronises the device: nothing may be finalised during the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # plans are made here, outside the capture
        eager = functions.fused_attention_step(g, q, k, v, dO).detach().clone()
    torch.cuda.current_stream().wait_stream(side)
    want = (eager, q.grad.clone(), k.grad.clone(), v.grad.clone())
    q.grad = k.grad = v.grad = None
    graph = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            o = functions.fused_attention_step(g, q, k, v, dO)
    finally:
        gc.enable()
    for _ in range(2):
        for x in (o, q.grad, k.grad, v.grad):
            x.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip((o, q.grad, k.grad, v.grad), want):
            assert torch.equal(x.detach(), y)
