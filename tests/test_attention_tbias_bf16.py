"""GPU tier of the bfloat16 fused attention step with an edge-type score bias (kernels_attn_tbias_bf16.h)
against the plain float64 reference of attention_bf16_opts_reference.py with b = B.double()[etype]; dB is the index_add
of its db.  Tolerances: test_attention_bf16.py's BF_TOL for o, dQ, dK, dV and the fp32 TOL for stats; for dB BF_TOL's
rtol with atol = the fp32 atol times sqrt(n_max), n_max the largest edge count of one type (4.5p's rule)."""
import ctypes

import pytest
import torch

import attention_bf16_opts_reference as R
from custom_op_benchmark_amd import functions, graphop as ops
from test_attention_bf16 import BF, BF_TOL, F32, HD, SB_PAIRS, _edge_graphs, _inputs, _spread_inputs
from test_attention_bf16_opts import OFFSET, SEED, _permuted
from test_fused_attention import prof_tags

pytestmark = pytest.mark.gpu

TAGS = {"attn_tbias_bf16_" + t for t in ("fwd_rows", "fwd_merge", "pack", "rows_row", "rows_col", "bwd_merge", "db_reduce")}


def _table(n_edges, T, h, seed):
    """B (T, h) bfloat16 and int32 types by edge id"""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(T, h, generator=gen).to(BF), torch.randint(0, T, (n_edges,), generator=gen, dtype=torch.int32)


def _step(a8, inp, B, et, dev, p, head0=0, need_dB=True):
    """the raw ops -> o, stats, dQ, dK, dV, dB"""
    Q, K, V, dO = (x.to(dev) for x in inp)
    B, et, dr = B.to(dev), et.to(dev), (p, SEED, OFFSET, head0)
    o, stats = ops.attention_tbias_bf16_forward(*a8[:4], Q, K, V, B, et, *dr)
    return (o, stats, *ops.attention_tbias_bf16_backward(*a8, Q, K, V, B, et, o, stats, dO, *dr, need_dB))


def _check(g, src, dst, inp, B, et, got, p, what, head0=0, need_dB=True):
    Q, K, V, dO = inp
    o, stats, dQ, dK, dV, dB = (x.cpu() for x in got)
    assert o.dtype == dQ.dtype == dK.dtype == dV.dtype == dB.dtype == BF and stats.dtype == torch.float32
    T = B.size(0)
    tc = torch.where((et < 0) | (et >= T), T - 1, et).long()          # min((unsigned) t, T - 1)
    b = B.double()[tc]
    mult = R.multipliers(src, dst, Q.size(1), p, SEED, OFFSET, head0)
    o0, m0, linv0, _ = R.forward(src, dst, g.n_src, Q, K, V, b, mult)
    live = torch.bincount(src, minlength=g.n_src) > 0
    torch.testing.assert_close(o.double(), o0, **BF_TOL, msg=lambda m: what + " o: " + m)
    torch.testing.assert_close(stats[live, :, 0].double(), m0[live], **F32, msg=lambda m: what + " m: " + m)
    torch.testing.assert_close(stats[..., 1].double(), linv0, **F32, msg=lambda m: what + " 1/l: " + m)
    assert not o[~live].any() and not stats[~live].any() and not dQ[~live].any()
    dQ0, dK0, dV0, db0 = R.backward(src, dst, Q, K, V, o, dO, b, mult)
    for name, x, x0 in zip(("dQ", "dK", "dV"), (dQ, dK, dV), (dQ0, dK0, dV0)):
        torch.testing.assert_close(x.double(), x0, **BF_TOL, msg=lambda m: "%s %s: %s" % (what, name, m))
    if not need_dB:
        assert tuple(dB.shape) == (0,)
        return
    counts = torch.bincount(tc, minlength=T)
    dB0 = torch.zeros(T, Q.size(1), dtype=torch.float64).index_add_(0, tc, db0)
    torch.testing.assert_close(dB.double(), dB0, rtol=BF_TOL["rtol"], atol=F32["atol"] * float(counts.max()) ** 0.5,
                               msg=lambda m: what + " dB: " + m)
    assert dB.shape == B.shape and not dB[counts == 0].any()          # exactly 0 for types no edge carries


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("h,d", HD)
def test_every_pair(dev, h, d, p):
    g, src, dst = _permuted()
    inp = _inputs(g, h, d, seed=h * 100 + d)
    B, et = _table(g.n_edges, 5, h, seed=h + d)
    a8 = tuple(x.to(dev) for x in g.csr_args())
    got = _step(a8, inp, B, et, dev, p)
    _check(g, src, dst, inp, B, et, got, p, "p=%g h=%d d=%d" % (p, h, d))
    if p:          # stats are those of the undropped scores, bit for bit
        assert torch.equal(got[1], _step(a8, inp, B, et, dev, 0.0)[1])
    assert TAGS <= prof_tags(lambda: _step(a8, inp, B, et, dev, p))


@pytest.mark.parametrize("at_bound", [False, True])
@pytest.mark.parametrize("h,d", [(4, 16), (8, 32), (8, 64)])
def test_one_type_and_the_table_at_the_bound(dev, h, d, at_bound):
    """one type: all of a lane group's adds hit one word per head; 512 / h types: the row pass's LDS at its largest"""
    g, src, dst = _permuted()
    T = 512 // h if at_bound else 1
    inp = _inputs(g, h, d, seed=T)
    B, et = _table(g.n_edges, T, h, seed=d)
    a8 = tuple(x.to(dev) for x in g.csr_args())
    _check(g, src, dst, inp, B, et, _step(a8, inp, B, et, dev, 0.5), 0.5, "T=%d h=%d d=%d" % (T, h, d))
    if at_bound:
        B, et = _table(g.n_edges, T + 1, h, seed=d)
        with pytest.raises(RuntimeError, match=r"n_types \* h = %d is above 512" % (512 + h)):
            _step(a8, inp, B, et, dev, 0.5)
        with pytest.raises(RuntimeError, match=r"n_types \* h = %d is above 512" % (512 + h)):
            Q, K, V, dO = (x.to(dev) for x in inp)
            stats = torch.zeros(g.n_src, h, 2, device=dev)
            ops.attention_tbias_bf16_backward(*a8, Q, K, V, B.to(dev), et.to(dev), Q, stats, dO)


@pytest.mark.parametrize("need_dB", [True, False])
@pytest.mark.parametrize("name", ["tails", "repeated"])
@pytest.mark.parametrize("h,d,sb", SB_PAIRS)
def test_batch_tails_and_parallel_edges(dev, h, d, sb, name, need_dB):
    """identity edge ids (the kernels' NULL eid); parallel edges share one keep decision and differ in type"""
    for g, what in _edge_graphs(name, sb):
        inp = _spread_inputs(g, h, d, seed=h + d)
        B, et = _table(g.n_edges, 3, h, seed=sb)
        a8 = tuple(x.to(dev) for x in g.csr_args())
        got = _step(a8, inp, B, et, dev, 0.5, need_dB=need_dB)
        _check(g, g.src, g.dst, inp, B, et, got, 0.5, "%s h=%d d=%d %s" % (name, h, d, what), need_dB=need_dB)


def test_without_dB_the_partial_tables_stay_untouched(dev):
    """the C entry point with a caller-owned workspace whose last part, the partial tables, holds a sentinel"""
    h, d, T = 4, 16, 6
    g, src, dst = _permuted()
    a8 = tuple(x.to(dev) for x in g.csr_args())
    Q, K, V, dO = (x.to(dev) for x in _inputs(g, h, d, seed=1))
    B, et = (x.to(dev) for x in _table(g.n_edges, T, h, seed=2))
    o, stats = ops.attention_tbias_bf16_forward(*a8[:4], Q, K, V, B, et)
    want = ops.attention_tbias_bf16_backward(*a8, Q, K, V, B, et, o, stats, dO, need_dB=False)
    pr, pc = ops.get_plan(*a8[:4], g.n_dst), ops.get_plan(*a8[4:], g.n_src)
    sizes = (g.n_edges, g.n_src, g.n_dst, h, d)
    plain = ops._workspace(Q, None, True, *sizes, pr, pc)[1]
    ws, nbytes = ops._attn_edge_workspace(Q, True, sizes + (T,), pr, pc, "tbias", bf16=True)
    assert nbytes > plain and (nbytes - plain) % 256 == 0
    ws[plain:] = 0xA5
    out = [torch.empty_like(x) for x in (Q, K, V)]
    ptr = ops.ptr
    ops.check(ops.lib().graphop_attention_tbias_bf16_backward(
        *(ptr(x) for x in a8), ptr(Q), ptr(K), ptr(V), ptr(B), ptr(et), ptr(o), ptr(stats), ptr(dO), *(ptr(x) for x in out),
        ctypes.c_void_p(0), a8[0].size(0), a8[4].size(0), *sizes, T, ptr(ws), nbytes, pr.handle, pc.handle,
        ops.stream_of(Q), 0.0, 0, 0, 0))
    assert bool((ws[plain:] == 0xA5).all())
    for x, y in zip(out, want):
        assert torch.equal(x, y)


def test_out_of_range_types_are_clamped(dev):
    h, d, T = 4, 32, 4
    g, src, dst = _permuted()
    inp = _inputs(g, h, d, seed=3)
    B, et = _table(g.n_edges, T, h, seed=4)
    et[::7], et[3::11], et[5::13] = -1, T, 2 ** 31 - 1
    buf = torch.full((3 * T * h,), 1e30, dtype=BF, device=dev)
    Bd = buf[T * h:2 * T * h].view(T, h).copy_(B)
    a8 = tuple(x.to(dev) for x in g.csr_args())
    got = _step(a8, inp, Bd, et, dev, 0.5)
    assert all(bool(torch.isfinite(x.float()).all()) for x in got)
    assert bool((buf[:T * h] == 1e30).all()) and bool((buf[2 * T * h:] == 1e30).all())
    _check(g, src, dst, inp, B, et, got, 0.5, "clamped")


def test_several_chunks_per_lane_group(dev):
    """the preconditions of test_attention_bf16.py's test of this name; two runs agree bit for bit, dB included"""
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
    B, et = _table(g.n_edges, 7, h, seed=3)
    a8 = tuple(x.to(dev) for x in g.csr_args())
    got = _step(a8, inp, B, et, dev, 0.5)
    _check(g, src, dst, inp, B, et, got, 0.5, "cpg=%d" % cpg)
    for x, y in zip(got, _step(a8, inp, B, et, dev, 0.5)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("head0", [0, 3])
@pytest.mark.parametrize("h,d", [(8, 8), (8, 32)])
def test_head0(dev, h, d, head0):
    g, src, dst = _permuted()
    inp = _inputs(g, h, d, seed=head0)
    B, et = _table(g.n_edges, 5, h, seed=1)
    a8 = tuple(x.to(dev) for x in g.csr_args())
    _check(g, src, dst, inp, B, et, _step(a8, inp, B, et, dev, 0.5, head0), 0.5, "head0=%d h=%d d=%d" % (head0, h, d), head0)


def test_autograd_class_on_bf16_leaves(dev):
    h, d = 4, 32
    g, src, dst = _permuted()
    a8 = tuple(x.to(dev) for x in g.csr_args())
    inp = _inputs(g, h, d, seed=5)
    B, et = _table(g.n_edges, 5, h, seed=6)
    want = _step(a8, inp, B, et, dev, 0.5)
    for b_grad in (True, False):
        q, k, v, dO = (x.to(dev).requires_grad_(i < 3) for i, x in enumerate(inp))
        Bl = B.to(dev).requires_grad_(b_grad)
        o = functions.FusedAttentionTypeBias.apply(*a8, q, k, v, Bl, et.to(dev), 0.5, SEED, OFFSET)
        o.backward(dO)
        for x, y in zip((o.detach(), q.grad, k.grad, v.grad), (want[0],) + want[2:5]):
            assert x.dtype == BF and torch.equal(x, y)
        if b_grad:
            assert Bl.grad.dtype == BF and Bl.grad.shape == B.shape and torch.equal(Bl.grad, want[5])
        else:          # no dB is made: no reduce runs
            assert Bl.grad is None
            run = lambda: functions.FusedAttentionTypeBias.apply(*a8, q, k, v, Bl, et.to(dev), 0.5, SEED, OFFSET).backward(dO)
            assert "attn_tbias_bf16_db_reduce" not in prof_tags(run)
    # the compiled binding answers like the ctypes one
    ext = ops.cpp_ext
    assert ext is not None, "graphop_cpp.so not built (run __graft_entry__.build())"
    Q, K, V, dO = (x.to(dev) for x in inp)
    f1 = ext.attention_tbias_bf16_forward(*a8[:4], Q, K, V, B.to(dev), et.to(dev), p=0.5, seed=SEED, offset=OFFSET)
    b1 = ext.attention_tbias_bf16_backward(*a8, Q, K, V, B.to(dev), et.to(dev), *f1, dO, p=0.5, seed=SEED, offset=OFFSET)
    for x, y in zip(list(f1) + list(b1), want):
        assert torch.equal(x, y)
