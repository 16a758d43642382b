"""GPU tier of the bfloat16 fused attention step with edge features (kernels_attn_edge_bf16.h) against the
plain float64 reference of attention_edge_bf16_reference.py.  Tolerances: test_attention_bf16.py's BF_TOL (one bf16
rounding plus the fp32 TOL) for o, dQ, dK, dV, dxe, with atol / (1 - p) under dropout as attention_edge_reference.tol has
it; the fp32 TOL for stats.  Inputs are the fp32 edge tests' scales: Q, dO ~ randn / sqrt(d), K, V, xe ~ randn."""
import pytest
import torch

import attention_edge_bf16_reference as R
from custom_op_benchmark_amd import functions, graphop as ops
from test_attention_bf16 import BF, BF_TOL, F32, HD, _edge_graphs, _spread_inputs
from test_attention_bf16_opts import OFFSET, SEED, _permuted
from test_fused_attention import prof_tags

pytestmark = pytest.mark.gpu

TAGS = {"attn_edge_bf16_" + t for t in ("fwd_rows", "fwd_merge", "pack", "rows_row", "rows_col", "bwd_merge")}
SB_PAIRS = [(4, 16, 8), (4, 64, 4), (8, 64, 1)]          # (h, d, EdgeBf16Cfg<h, d>::SB): one pair per batch size


def _inputs(g, h, d, seed):
    """(Q, K, V, dO, xe) in bfloat16"""
    gen = torch.Generator().manual_seed(seed)
    Q, K, V, dO = (torch.randn(n, h, d, generator=gen) for n in (g.n_src, g.n_dst, g.n_dst, g.n_src))
    xe = torch.randn(g.n_edges, h, d, generator=gen)
    return (Q / d ** 0.5).to(BF), K.to(BF), V.to(BF), (dO / d ** 0.5).to(BF), xe.to(BF)


def _xe(g, h, d, seed):
    return torch.randn(g.n_edges, h, d, generator=torch.Generator().manual_seed(seed)).to(BF)


def _step(a8, inp, dev, p, head0=0, need_dxe=True):
    """the raw ops -> o, stats, dQ, dK, dV, dxe"""
    Q, K, V, dO, xe = (x.to(dev) for x in inp)
    dr = (p, SEED, OFFSET, head0)
    o, stats = ops.attention_edge_bf16_forward(*a8[:4], Q, K, V, xe, *dr)
    return (o, stats, *ops.attention_edge_bf16_backward(*a8, Q, K, V, xe, o, stats, dO, *dr, need_dxe))


def _check(g, src, dst, inp, got, p, what, head0=0, need_dxe=True):
    Q, K, V, dO, xe = inp
    o, stats, dQ, dK, dV, dxe = (x.cpu() for x in got)
    assert o.dtype == dQ.dtype == dK.dtype == dV.dtype == dxe.dtype == BF and stats.dtype == torch.float32
    tol = dict(rtol=BF_TOL["rtol"], atol=BF_TOL["atol"] / (1 - p))
    mult = R.multipliers(src, dst, Q.size(1), p, SEED, OFFSET, head0)
    o0, m0, linv0 = R.forward(src, dst, g.n_src, Q, K, V, xe, mult)
    live = torch.bincount(src, minlength=g.n_src) > 0
    torch.testing.assert_close(o.double(), o0, **tol, msg=lambda m: what + " o: " + m)
    torch.testing.assert_close(stats[live, :, 0].double(), m0[live], **F32, msg=lambda m: what + " m: " + m)
    torch.testing.assert_close(stats[..., 1].double(), linv0, **F32, msg=lambda m: what + " 1/l: " + m)
    assert not o[~live].any() and not stats[~live].any() and not dQ[~live].any()
    want = R.backward(src, dst, Q, K, V, xe, o, dO, mult)
    for name, x, x0 in zip(("dQ", "dK", "dV"), (dQ, dK, dV), want):
        torch.testing.assert_close(x.double(), x0, **tol, msg=lambda m: "%s %s: %s" % (what, name, m))
    if not need_dxe:
        assert tuple(dxe.shape) == (0,)
        return
    assert dxe.shape == xe.shape
    torch.testing.assert_close(dxe.double(), want[3], **tol, msg=lambda m: what + " dxe: " + m)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("h,d", HD)
def test_every_pair(dev, h, d, p):
    g, src, dst = _permuted()
    inp = _inputs(g, h, d, seed=h * 100 + d)
    a8 = tuple(x.to(dev) for x in g.csr_args())
    got = _step(a8, inp, dev, p)
    _check(g, src, dst, inp, got, p, "p=%g h=%d d=%d" % (p, h, d))
    if p:          # stats are those of the undropped scores, bit for bit
        assert torch.equal(got[1], _step(a8, inp, dev, 0.0)[1])
    assert TAGS <= prof_tags(lambda: _step(a8, inp, dev, p))


@pytest.mark.parametrize("need_dxe", [True, False])
@pytest.mark.parametrize("name", ["tails", "repeated"])
@pytest.mark.parametrize("h,d,sb", SB_PAIRS)
def test_batch_tails_and_parallel_edges(dev, h, d, sb, name, need_dxe):
    """identity edge ids (the kernels' NULL eid); parallel edges share one keep decision and have each their own xe row"""
    for g, what in _edge_graphs(name, sb):
        assert torch.equal(g.eid_r, torch.arange(g.n_edges))
        inp = _spread_inputs(g, h, d, seed=h + d) + (_xe(g, h, d, seed=sb),)
        a8 = tuple(x.to(dev) for x in g.csr_args())
        got = _step(a8, inp, dev, 0.5, need_dxe=need_dxe)
        _check(g, g.src, g.dst, inp, got, 0.5, "%s h=%d d=%d %s" % (name, h, d, what), need_dxe=need_dxe)


def test_several_chunks_per_lane_group(dev):
    """the preconditions of test_attention_bf16.py's test of this name; two runs agree bit for bit in all six outputs"""
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
    a8 = tuple(x.to(dev) for x in g.csr_args())
    got = _step(a8, inp, dev, 0.5)
    _check(g, src, dst, inp, got, 0.5, "cpg=%d" % cpg)
    for x, y in zip(got, _step(a8, inp, dev, 0.5)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("head0", [0, 3])
@pytest.mark.parametrize("h,d", [(8, 8), (8, 32)])
def test_head0(dev, h, d, head0):
    g, src, dst = _permuted()
    inp = _inputs(g, h, d, seed=head0)
    a8 = tuple(x.to(dev) for x in g.csr_args())
    _check(g, src, dst, inp, _step(a8, inp, dev, 0.5, head0), 0.5, "head0=%d h=%d d=%d" % (head0, h, d), head0)


def test_xe_and_dxe_inside_a_larger_buffer(dev):
    """xe and dxe are the middle thirds of buffers filled with 1e30: the margins stay untouched, every result is finite"""
    h, d = 4, 32
    g, src, dst = _permuted()
    inp = _inputs(g, h, d, seed=3)
    n = g.n_edges * h * d
    a8 = tuple(x.to(dev) for x in g.csr_args())
    Q, K, V, dO = (x.to(dev) for x in inp[:4])
    xbuf, gbuf = (torch.full((3 * n,), 1e30, dtype=BF, device=dev) for _ in range(2))
    xe = xbuf[n:2 * n].view(g.n_edges, h, d).copy_(inp[4])
    dxe = gbuf[n:2 * n].view(g.n_edges, h, d)
    dr = (0.5, SEED, OFFSET, 0)
    o, stats = ops.attention_edge_bf16_forward(*a8[:4], Q, K, V, xe, *dr)
    pr, pc = ops.get_plan(*a8[:4], g.n_dst), ops.get_plan(*a8[4:], g.n_src)
    sizes = (g.n_edges, g.n_src, g.n_dst, h, d)
    ws, nbytes = ops._attn_edge_workspace(Q, True, sizes, pr, pc, "edge", bf16=True)
    out = [torch.empty_like(x) for x in (Q, K, V)]
    ptr = ops.ptr
    ops.check(ops.lib().graphop_attention_edge_bf16_backward(
        *(ptr(x) for x in a8), ptr(Q), ptr(K), ptr(V), ptr(xe), ptr(o), ptr(stats), ptr(dO), *(ptr(x) for x in out), ptr(dxe),
        a8[0].size(0), a8[4].size(0), *sizes, ptr(ws), nbytes, pr.handle, pc.handle, ops.stream_of(Q), *dr))
    got = (o, stats, *out, dxe)
    assert all(bool(torch.isfinite(x.float()).all()) for x in got)
    for buf in (xbuf, gbuf):
        assert bool((buf[:n] == 1e30).all()) and bool((buf[2 * n:] == 1e30).all())
    _check(g, src, dst, inp, got, 0.5, "inside a buffer")


def test_classes_and_refusals(dev):
    h, d = 4, 32
    g, src, dst = _permuted()
    a8 = tuple(x.to(dev) for x in g.csr_args())
    inp = _inputs(g, h, d, seed=5)
    want = _step(a8, inp, dev, 0.5)
    for x_grad in (True, False):
        q, k, v = (x.to(dev).requires_grad_(True) for x in inp[:3])
        dO, xl = inp[3].to(dev), inp[4].to(dev).requires_grad_(x_grad)
        o = functions.FusedAttentionEdge.apply(*a8, q, k, v, xl, 0.5, SEED, OFFSET)
        o.backward(dO)
        for x, y in zip((o.detach(), q.grad, k.grad, v.grad), (want[0],) + want[2:5]):
            assert x.dtype == BF and torch.equal(x, y)
        if x_grad:
            assert xl.grad.dtype == BF and xl.grad.shape == xl.shape and torch.equal(xl.grad, want[5])
        else:
            assert xl.grad is None
    # the compiled binding answers like the ctypes one
    ext = ops.cpp_ext
    assert ext is not None, "graphop_cpp.so not built (run __graft_entry__.build())"
    Q, K, V, dO, xe = (x.to(dev) for x in inp)
    f1 = ext.attention_edge_bf16_forward(*a8[:4], Q, K, V, xe, p=0.5, seed=SEED, offset=OFFSET)
    b1 = ext.attention_edge_bf16_backward(*a8, Q, K, V, xe, *f1, dO, p=0.5, seed=SEED, offset=OFFSET)
    for x, y in zip(list(f1) + list(b1), want):
        assert torch.equal(x, y)
    assert tuple(ext.attention_edge_bf16_backward(*a8, Q, K, V, xe, *f1, dO, need_dxe=False)[3].shape) == (0,)
    # refusals: a pair outside the set, fp32 tensors, and the fp32 op on bfloat16 tensors
    q3, k3, x3 = (torch.zeros(n, 3, 8, dtype=BF, device=dev) for n in (g.n_src, g.n_dst, g.n_edges))
    with pytest.raises(RuntimeError, match="is not in the bfloat16 set"):
        ops.attention_edge_bf16_forward(*a8[:4], q3, k3, k3, x3)
    for mod in (ops, ext):
        with pytest.raises(RuntimeError, match="bfloat16 tensors only"):
            mod.attention_edge_bf16_forward(*a8[:4], Q.float(), K.float(), V.float(), xe.float())
    with pytest.raises(RuntimeError, match="float32 / float64"):
        ops.attention_edge_forward(*a8[:4], Q, K, V, xe)
