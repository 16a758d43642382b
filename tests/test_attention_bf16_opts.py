"""GPU tier of the bfloat16 fused attention step with attention dropout and a per-edge score bias
(kernels_attn_bf16_opts.h) against the plain float64 reference of attention_bf16_opts_reference.py.
Tolerances are test_attention_bf16.py's: BF_TOL = one bf16 rounding plus the fp32 TOL for every bf16 output, db included;
the fp32 TOL alone for stats."""
import functools
import gc

import pytest
import torch

import attention_bf16_opts_reference as R
from custom_op_benchmark_amd import functions, graphop as ops
from gat_edge_reference import permute_edge_ids
from test_attention_bf16 import BF, BF_TOL, F32, HD, SB_PAIRS, _edge_graphs, _graph, _inputs, _spread_inputs
from test_fused_attention import prof_tags, shuffled_chunk_arrays
from util import random_graph

pytestmark = pytest.mark.gpu

MODES = {"dropout": (0.5, False), "bias": (0.0, True), "both": (0.5, True)}          # mode: (p, with b)
SEED, OFFSET = 2 ** 40 + 12345, 7
TAGS = {"attn_bf16_opts_fwd_rows", "attn_bf16_opts_fwd_merge", "attn_bf16_opts_pack", "attn_bf16_opts_rows_row",
        "attn_bf16_opts_rows_col", "attn_bf16_opts_bwd_merge"}


@functools.lru_cache(maxsize=None)
def _permuted(big=False):
    """(g, src, dst): a graph whose edge ids are the slot order in neither orientation, and its edges in edge-id order"""
    g = random_graph(3000, 3000, 110000, seed=17, chunk_size=1) if big else _graph()
    g, src, dst = permute_edge_ids(g, seed=5)
    ar = torch.arange(g.n_edges)
    assert not torch.equal(g.eid_r, ar) and not torch.equal(g.eid_c, ar)
    return g, src, dst


def _bias(n_edges, h, seed):
    return torch.randn(n_edges, h, generator=torch.Generator().manual_seed(seed)).to(BF)


def _step(a8, inp, b, dev, p, head0=0, need_db=True):
    """the raw ops -> o, stats, dQ, dK, dV, db"""
    Q, K, V, dO = (x.to(dev) for x in inp)
    b = None if b is None else b.to(dev)
    dr = (p, SEED, OFFSET, head0)
    o, stats = ops.attention_bf16_opts_forward(*a8[:4], Q, K, V, b, *dr)
    return (o, stats, *ops.attention_bf16_opts_backward(*a8, Q, K, V, b, o, stats, dO, *dr, need_db))


def _check(g, src, dst, inp, b, got, p, what, head0=0, need_db=True):
    Q, K, V, dO = inp
    o, stats, dQ, dK, dV, db = (x.cpu() for x in got)
    assert o.dtype == dQ.dtype == dK.dtype == dV.dtype == db.dtype == BF and stats.dtype == torch.float32
    mult = R.multipliers(src, dst, Q.size(1), p, SEED, OFFSET, head0)
    o0, m0, linv0, _ = R.forward(src, dst, g.n_src, Q, K, V, b, mult)
    live = torch.bincount(src, minlength=g.n_src) > 0
    torch.testing.assert_close(o.double(), o0, **BF_TOL, msg=lambda m: what + " o: " + m)
    torch.testing.assert_close(stats[live, :, 0].double(), m0[live], **F32, msg=lambda m: what + " m: " + m)
    torch.testing.assert_close(stats[..., 1].double(), linv0, **F32, msg=lambda m: what + " 1/l: " + m)
    assert not o[~live].any() and not stats[~live].any() and not dQ[~live].any()
    cold = torch.bincount(dst, minlength=g.n_dst) == 0
    assert not dK[cold].any() and not dV[cold].any()
    want = R.backward(src, dst, Q, K, V, o, dO, b, mult)
    if b is None or not need_db:
        assert db.numel() == 0
        want, db = want[:3], None
    for name, x, x0 in zip(("dQ", "dK", "dV", "db"), (dQ, dK, dV, db), want):
        torch.testing.assert_close(x.double(), x0, **BF_TOL, msg=lambda m: "%s %s: %s" % (what, name, m))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("h,d", HD)
def test_every_pair_every_mode(dev, h, d, mode):
    p, biased = MODES[mode]
    g, src, dst = _permuted()
    inp = _inputs(g, h, d, seed=h * 100 + d)
    b = _bias(g.n_edges, h, seed=h + d) if biased else None
    a8 = tuple(x.to(dev) for x in g.csr_args())
    got = _step(a8, inp, b, dev, p)
    _check(g, src, dst, inp, b, got, p, "%s h=%d d=%d" % (mode, h, d))
    if p:          # stats are those of the undropped scores, bit for bit
        assert torch.equal(got[1], _step(a8, inp, b, dev, 0.0)[1])
    assert TAGS <= prof_tags(lambda: _step(a8, inp, b, dev, p))


@pytest.mark.parametrize("head0", [0, 3, 5])
@pytest.mark.parametrize("h,d", [(8, 8), (4, 16), (8, 32)])
def test_head0(dev, h, d, head0):
    """lane groups of 8 where one lane makes every Philox call (three at 8 x 8 with head0 % 4 != 0), blocks that start
    before head0 and move down, and lane groups of 16 where a slot's lanes share the calls"""
    g, src, dst = _permuted()
    inp = _inputs(g, h, d, seed=head0)
    b = _bias(g.n_edges, h, seed=1)
    a8 = tuple(x.to(dev) for x in g.csr_args())
    _check(g, src, dst, inp, b, _step(a8, inp, b, dev, 0.5, head0), 0.5, "head0=%d h=%d d=%d" % (head0, h, d), head0)


def test_several_chunks_per_lane_group(dev):
    """the preconditions of test_attention_bf16.py's test of this name, both options; two runs agree bit for bit"""
    h, d = 4, 16
    g, src, dst = _permuted(big=True)
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
    b = _bias(g.n_edges, h, seed=3)
    a8 = tuple(x.to(dev) for x in g.csr_args())
    got = _step(a8, inp, b, dev, 0.5)
    _check(g, src, dst, inp, b, got, 0.5, "cpg=%d" % cpg)
    for x, y in zip(got, _step(a8, inp, b, dev, 0.5)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("need_db", [True, False])
@pytest.mark.parametrize("name", ["tails", "repeated"])
@pytest.mark.parametrize("h,d,sb", SB_PAIRS)
def test_batch_tails_and_parallel_edges(dev, h, d, sb, name, need_db):
    """identity edge ids (the kernels' NULL eid); parallel edges share one keep decision and have their own b and db"""
    for g, what in _edge_graphs(name, sb):
        inp = _spread_inputs(g, h, d, seed=h + d)
        b = _bias(g.n_edges, h, seed=sb)
        a8 = tuple(x.to(dev) for x in g.csr_args())
        got = _step(a8, inp, b, dev, 0.5, need_db=need_db)
        _check(g, g.src, g.dst, inp, b, got, 0.5, "%s h=%d d=%d %s" % (name, h, d, what), need_db=need_db)


def test_identities_and_surface(dev):
    h, d = 4, 32
    g, src, dst = _permuted()
    gd = g.to(dev)
    a8 = gd.csr_args()
    inp = _inputs(g, h, d, seed=5)
    Q, K, V, dO = (x.to(dev) for x in inp)
    o, stats = ops.attention_forward(*a8[:4], Q, K, V)
    plain = (o, stats, *ops.attention_backward(*a8, Q, K, V, o, stats, dO))
    for x, y in zip(_step(a8, inp, None, dev, 0.0)[:5], plain):          # no option: the plain step
        assert torch.equal(x, y)
    zero = torch.zeros(g.n_edges, h, dtype=BF)
    got = _step(a8, inp, zero, dev, 0.0)
    for x, y in zip(got[:5], plain):          # b = 0 adds exact zeros
        assert torch.equal(x, y)
    torch.testing.assert_close(got[5].cpu().double(), R.backward(src, dst, *inp[:3], got[0].cpu(), inp[3], zero)[3], **BF_TOL)
    b = _bias(g.n_edges, h, seed=9)
    full = _step(a8, inp, b, dev, 0.5)
    for x, y in zip(_step(a8, inp, b, dev, 0.5, need_db=False)[:5], full[:5]):
        assert torch.equal(x, y)
    # the autograd classes make one call with head0 = 0 and return bf16 gradients
    bd = b.to(dev)
    for cls, extra, want in ((functions.FusedAttentionDropout, (), _step(a8, inp, None, dev, 0.5)),
                             (functions.FusedAttentionBias, (bd.clone().requires_grad_(True),), full)):
        q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
        oc = cls.apply(*a8, q, k, v, *extra, 0.5, SEED, OFFSET)
        oc.backward(dO)
        grads = [q.grad, k.grad, v.grad] + [x.grad for x in extra]
        assert all(x.dtype == BF for x in grads)
        for x, y in zip([oc.detach()] + grads, [want[0]] + list(want[2:])):
            assert torch.equal(x, y)
    # the compiled binding answers like the ctypes one
    ext = ops.cpp_ext
    assert ext is not None, "graphop_cpp.so not built (run __graft_entry__.build())"
    f1 = ext.attention_bf16_opts_forward(*a8[:4], Q, K, V, bd, p=0.5, seed=SEED, offset=OFFSET)
    b1 = ext.attention_bf16_opts_backward(*a8, Q, K, V, bd, *f1, dO, p=0.5, seed=SEED, offset=OFFSET)
    for x, y in zip(list(f1) + list(b1), full):
        assert torch.equal(x, y)
    assert ext.attention_bf16_opts_backward(*a8, Q, K, V, None, *f1, dO, p=0.5, seed=SEED)[3].numel() == 0
    # unsupported: an error that names the condition, never an upcast
    odd = [torch.zeros(n, 3, 8, dtype=BF, device=dev) for n in (g.n_src, g.n_dst, g.n_dst)]
    with pytest.raises(RuntimeError, match=r"\(h, d\) = \(3, 8\) is not in the bfloat16 set"):
        functions.FusedAttentionDropout.apply(*a8, *odd, 0.5, SEED)
    shuffled = tuple(x.to(dev) for x in shuffled_chunk_arrays(g, seed=11))
    with pytest.raises(RuntimeError, match="not row_owned"):
        functions.FusedAttentionBias.apply(*shuffled, Q, K, V, bd)
    with pytest.raises(RuntimeError, match="bfloat16 tensors only"):
        ops.attention_bf16_opts_forward(*a8[:4], Q.float(), K.float(), V.float())


def test_step_replays_from_a_hip_graph(dev):
    g = _permuted()[0].to(dev)
    Q, K, V, dO = (x.to(dev) for x in _inputs(g, 8, 32, seed=6))
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
    b = _bias(g.n_edges, 8, seed=7).to(dev).requires_grad_(True)
    step = lambda: functions.fused_attention_bias_step(g, q, k, v, b, dO, 0.5, SEED, OFFSET)
    leaves = (q, k, v, b)
    gc.collect()          # (freeing a plan synchronises the device: nothing may be finalised during the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # plans are made here, outside the capture
        eager = step().detach().clone()
    torch.cuda.current_stream().wait_stream(side)
    want = (eager, *(x.grad.clone() for x in leaves))
    for x in leaves:
        x.grad = None
    graph = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            o = step()
    finally:
        gc.enable()
    for _ in range(2):
        for x in (o, *(x.grad for x in leaves)):
            x.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip((o, *(x.grad for x in leaves)), want):
            assert torch.equal(x.detach(), y)
