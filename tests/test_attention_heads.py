"""GPU tier of the several-head forms of the fused dot-product attention ops (kernels_attn_heads.h):
graphop.attention_forward / _dropout_ / _bias_ with h > 1 heads in ONE call, and the three autograd classes on top of
them, against the float64 CPU statements of the definition (tests/attention_bias_reference.py,
tests/attention_dropout_reference.py), against the composed path and against the head-grouped calls.  The form is
forced with the knob attn_heads = 1 and asserted through the profile tags.

Tolerances are TOL of tests/test_fused_attention.py (fp32 rtol 1e-4 / atol 1e-5) with atol times 1 / (1 - p), as
test_attention_bias.py::_compare applies them; two fp32 results compared with each other get twice that.  Graphs:
random_graph(300, 337, 2700, chunk_size=8, zero_rows=0.2, hub=150) -- rectangular, rows without edges, a hub row cut
into many chunks and so split over lane groups, parallel edges."""
import functools

import pytest
import torch

import attention_dropout_reference as A
import gat_edge_reference as GE
import oracle
from custom_op_benchmark_amd import _lib, functions, graphs, graphop as ops
from test_attention_bias import (_class_step, _compare, _compare_stats, _dev8, _device, _inputs, _reference,
                                 _unsplit_graph, _without_bias)
from test_fused_attention import close, prof_tags, shuffled_chunk_arrays
from util import oracle_step, rand_inputs, random_graph

pytestmark = pytest.mark.gpu

HD = [(2, 32), (2, 64), (4, 16), (4, 32), (4, 64), (8, 8), (8, 16), (8, 32)]   # the several-head pairs of GO_DISPATCH_GAT_HD
DROP = (0.6, 1234567890123, 7)
NONE = (0.0, 0, 0)
BWD = {"attn_heads_rows_row", "attn_heads_rows_col"}
NEW = BWD | {"attn_heads_fwd_rows"}
COMPOSED = {"attn_bias_add", "sddmm_fwd", "softmax_fwd", "spmm_fwd", "attn_drop_apply"}
F32 = torch.float32


@pytest.fixture
def heads_on():
    _lib.tune("attn_heads", 1); _lib.clear_plan_cache()
    yield
    _lib.tune_reset(); _lib.clear_plan_cache()


@functools.lru_cache(maxsize=None)
def _graph(seed=3):
    g = random_graph(300, 337, 2700, seed=seed, chunk_size=8, zero_rows=0.2, hub=150)
    deg = torch.bincount(g.src, minlength=g.n_src)
    assert g.n_src != g.n_dst and (deg == 0).any() and deg.max() >= 150 and (deg % 8 != 0).any()
    assert torch.unique(torch.stack([g.src, g.dst], 1), dim=0).size(0) < g.n_edges          # parallel edges
    return g


@functools.lru_cache(maxsize=None)
def _case(h, d, p):
    """(graph, inputs, float64 reference) of test 1, computed once for both chunk orders"""
    g = _graph()
    inp = _inputs(g, h, d, F32, seed=h * 100 + d)
    drop = DROP if p > 0 else NONE
    return g, inp, _reference(g, inp, *drop)


# ---- 1. every (h, d) of the set ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.6])
@pytest.mark.parametrize("rows_sorted", [True, False])
@pytest.mark.parametrize("h,d", HD)
def test_every_shape_matches_the_reference(dev, heads_on, h, d, rows_sorted, p):
    """With a bias: o, the statistics of the rows with edges, dQ, dK, dV and db against the float64 reference; the three
    new passes ran and nothing of the composed path did.  With the chunk list shuffled no row is owned, the backward
    still runs its two fused passes and only the forward composes."""
    g, inp, want = _case(h, d, p)
    drop = DROP if p > 0 else NONE
    a8 = _dev8(g.csr_args() if rows_sorted else shuffled_chunk_arrays(g, seed=11), dev)
    got = _device(a8, dev, inp, *drop)
    tags = prof_tags(lambda: _device(a8, dev, inp, *drop))
    if rows_sorted:
        assert NEW <= tags and not (COMPOSED & tags), tags
    else:
        assert BWD <= tags and "attn_heads_fwd_rows" not in tags and "attn_bias_add" in tags, tags
    what = "h=%d d=%d p=%g sorted=%d " % (h, d, p, rows_sorted)
    _compare(got, want, F32, p, what)
    _compare_stats(g, got, want, F32, what, empty_zero=rows_sorted)
    if rows_sorted:
        assert not got["o"].cpu()[torch.bincount(g.src, minlength=g.n_src) == 0].any()


# ---- 2. heads do not leak into each other ------------------------------------------------------------------------------
def test_heads_do_not_leak_into_each_other(dev, heads_on):
    """h = 4, d = 16: the heads' scores live on four scales a factor 10 apart (Q[:, k] *= 10 ** k), b is drawn per head
    and head 2's is shifted by +50 on one edge of every row: a maximum, a sum or a weight taken from a neighbouring
    head's lanes would be off by orders of magnitude.  Every output and the statistics are compared head by head.
    The base scale of Q: a weight exp(s - m) has the RELATIVE error of its score's ABSOLUTE error, and an fp32 score of
    d = 16 products carries about 2 ** -23 sqrt(d) |s|, so rtol 1e-4 with a margin of ten wants |s| below a few tens at
    the largest scale.  Q = randn / sqrt(d) / 30 puts head 3's scores at std 8 (largest ~30) and head 0's at 0.008.
    (With Q = randn / sqrt(d), head 3's scores reach ~1000 and one ulp of a score is 6e-5: no fp32 form can hold rtol
    1e-4 there; measured: 8 of 5392 elements of head 3's dK over tolerance on these kernels and 3 on the composed
    path, the largest error 2.3e-4 on both, heads 0 to 2 within tolerance on both.)"""
    h, d = 4, 16
    g = _graph()
    Q, K, V, b, dO = _inputs(g, h, d, F32, seed=21)
    Q = Q / 30 * (10.0 ** torch.arange(h, dtype=F32))[None, :, None]
    first = torch.full((g.n_src,), g.n_edges, dtype=torch.int64).scatter_reduce(
        0, g.src, torch.arange(g.n_edges), "amin")          # the lowest edge id of every row with edges
    b = b.clone()
    b[first[first < g.n_edges], 2] += 50.0
    inp = (Q, K, V, b, dO)
    a8 = _dev8(g.csr_args(), dev)
    for drop in (NONE, DROP):
        want = _reference(g, inp, *drop)
        got = _device(a8, dev, inp, *drop)
        assert NEW <= prof_tags(lambda: _device(a8, dev, inp, *drop))
        has = torch.bincount(g.src, minlength=g.n_src) > 0
        for k in range(h):
            what = "head %d p=%g " % (k, drop[0])
            _compare({n: got[n][:, k] for n in ("o", "dQ", "dK", "dV", "db")},
                     {n: want[n][:, k] for n in ("o", "dQ", "dK", "dV", "db")}, F32, drop[0], what)
            _compare(dict(stats=got["stats"].cpu()[has][:, k]), dict(stats=want["stats"][has][:, k]), F32, 0.0, what,
                     keys=("stats",))


# ---- 3. without a bias and without dropout -------------------------------------------------------------------------------
def test_plain_op_vs_oracle_and_is_fused(dev):
    """graphop_attention_forward / _backward at 8 x 32 against the oracle's composed step (as
    test_fused_head_groups_vs_oracle compares); attention_backward_is_fused follows the knob."""
    h, d = 8, 32
    g = _graph()
    inp = rand_inputs(g, h, d, seed=5, normal=True)
    dO = inp["dO"][:g.n_src]
    want = oracle_step(oracle, g, inp["Q"], inp["K"], inp["V"], torch.cat([dO, torch.zeros(g.n_dst - g.n_src, h, d)]))
    a8 = _dev8(g.csr_args(), dev)
    Q, K, V, dOd = (x.to(dev) for x in (inp["Q"], inp["K"], inp["V"], dO))

    def step():
        o, stats = ops.attention_forward(*a8[:4], Q, K, V)
        return (o,) + tuple(ops.attention_backward(*a8, Q, K, V, o, stats, dOd))

    try:
        _lib.tune("attn_heads", 1); _lib.clear_plan_cache()
        assert ops.attention_backward_is_fused(*a8, Q, K) is True
        tags = prof_tags(step)
        assert NEW <= tags and not (COMPOSED & tags), tags
        o, dQ, dK, dV = step()
        close(o, want["o"][:g.n_src])
        for got, k in ((dQ, "dQ"), (dK, "dK"), (dV, "dV")):
            close(got, want[k])
        _lib.tune("attn_heads", 0); _lib.clear_plan_cache()
        assert ops.attention_backward_is_fused(*a8, Q, K) is False
        assert not (NEW & prof_tags(step))
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()


# ---- 4. b = 0, need_db = False ----------------------------------------------------------------------------------------------
def test_zero_bias_and_need_db_false(dev, heads_on):
    plain_keys = ("o", "dQ", "dK", "dV", "stats")
    g = _graph()
    a8 = _dev8(g.csr_args(), dev)
    for h, d in ((4, 16), (8, 32)):
        inp = _inputs(g, h, d, F32, seed=d)
        zero = inp[:3] + (torch.zeros_like(inp[3]),) + inp[4:]
        for drop in (NONE, DROP):
            with_b, without = _device(a8, dev, zero, *drop), _without_bias(a8, dev, zero, *drop)
            _compare(with_b, without, F32, drop[0], "b=0 h=%d d=%d " % (h, d), factor=2, keys=plain_keys)
            # the hub row is summed by float atomics in any order: the two-results tolerance
            nodb = _device(a8, dev, inp, *drop, need_db=False)
            assert nodb["db"].numel() == 0
            _compare(nodb, _device(a8, dev, inp, *drop), F32, drop[0], "need_db=False ", factor=2, keys=plain_keys)
        assert NEW <= prof_tags(lambda: _without_bias(a8, dev, zero, *DROP))
        assert NEW <= prof_tags(lambda: _device(a8, dev, inp, *NONE, need_db=False))
    # no row and no column split over chunks: nothing is summed by atomics, need_db changes no other bit
    g = _unsplit_graph(3)
    a8 = _dev8(g.csr_args(), dev)
    for h, d in ((4, 16), (8, 32)):
        inp = _inputs(g, h, d, F32, seed=d)
        for drop in (NONE, DROP):
            x, y = _device(a8, dev, inp, *drop), _device(a8, dev, inp, *drop, need_db=False)
            for k in plain_keys:
                assert torch.equal(x[k], y[k]), (h, d, drop, k)
            assert y["db"].numel() == 0 and x["db"].shape == inp[3].shape


# ---- 5. b is addressed by edge id ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_sorted", [True, False])
@pytest.mark.parametrize("ids", ["row_identity", "column_identity", "permuted"])
def test_bias_is_addressed_by_edge_id_not_by_slot(dev, heads_on, ids, rows_sorted):
    """Row-major identity (the row pass takes eid == NULL, the column pass reads eid_c), column-major identity (the other
    way round) and a random renumbering (both read their arrays): b[e, k] and db[e, k] follow the edge ids."""
    h, d = 4, 16
    g0 = _graph(seed=9)
    g, src, dst = {"row_identity": lambda: (g0, g0.src, g0.dst), "column_identity": lambda: GE.column_identity_edge_ids(g0),
                   "permuted": lambda: GE.permute_edge_ids(g0, 5)}[ids]()
    assert torch.equal(g.eid_r, torch.arange(g.n_edges)) == (ids == "row_identity")
    inp = _inputs(g, h, d, F32, seed=6)
    a8 = _dev8(g.csr_args() if rows_sorted else shuffled_chunk_arrays(g, seed=13), dev)
    for drop in (NONE, DROP):
        got = _device(a8, dev, inp, *drop)
        want = _reference(g, inp, *drop, src=src, dst=dst)
        _compare(got, want, F32, drop[0], "%s p=%g " % (ids, drop[0]))          # db[e, k] included: its positions
    tags = prof_tags(lambda: _device(a8, dev, inp, *DROP))
    assert BWD <= tags and ("attn_heads_fwd_rows" in tags) == rows_sorted, tags
    if ids != "row_identity":          # the same b read by slot instead would be another result
        other = _device(_dev8(g0.csr_args(), dev), dev, inp, *NONE)
        assert not torch.allclose(other["o"], _device(a8, dev, inp, *NONE)["o"], rtol=1e-3, atol=1e-4)


# ---- 6. several chunks per lane group ----------------------------------------------------------------------------------------
def test_several_chunks_per_lane_group(dev, heads_on):
    """Chunks of one slot, enough of them that the launches' rule clamp(n_chunks / (n_cu * 16 * 4), 1, 16) gives cpg >= 2
    on this device, and no multiple of cpg: the last group's run is short.  Rows of ~37 chunks over groups of cpg: some
    groups lie wholly inside one row (one mid-row piece), most start inside one row and end inside another (first and
    last row both shared, two pieces), the rows between are stored whole."""
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
    inp = _inputs(g, h, d, F32, seed=2)
    a8 = _dev8(g.csr_args(), dev)
    got = _device(a8, dev, inp, *DROP)
    assert NEW <= prof_tags(lambda: _device(a8, dev, inp, *DROP))
    want = _reference(g, inp, *DROP)
    _compare(got, want, F32, DROP[0], "cpg=%d " % cpg)
    _compare_stats(g, got, want, F32, "cpg=%d " % cpg, empty_zero=True)


# ---- 7. head0 ------------------------------------------------------------------------------------------------------------------
def _kept(out, g, d, p):
    """The keep decisions (E, h) read back from a step with Q = K = 0, b = 0 and V = dO = 1: a_e = 1 / deg_i,
    o_i = S_i = sum_e a_e m_e in every component, D_i = d S_i and db_e = a_e d (m_e - S_i), so m_e = db_e deg_i / d + S_i is
    0 or 1 / (1 - p)."""
    deg = torch.bincount(g.src, minlength=g.n_src).double()
    m = out["db"].cpu().double() * deg[g.src][:, None] / d + out["o"].cpu().double()[g.src][:, :, 0]
    assert ((m.abs() < 1e-3) | ((m - 1 / (1 - p)).abs() < 1e-3)).all()
    return m > 0.5 / (1 - p)


def test_head0_names_the_global_heads(dev, heads_on):
    """Heads [2, 4) of an 8 x 16 problem called with head0 = 2 (two heads of d = 16: the composed path, as a head group
    is called) against slices [2:4] of the whole several-head call: the same dropout decisions, values at the
    two-results tolerance.  And with a several-head shape and a head0 that is no multiple of four (4 x 16 at head0 = 2:
    Philox blocks 0 and 1)."""
    g = _graph()
    a8 = _dev8(g.csr_args(), dev)
    p, seed, offset = DROP
    for h, d, g0, hg in ((8, 16, 2, 2), (8, 16, 2, 4)):
        inp = _inputs(g, h, d, F32, seed=31)
        part = tuple(x[:, g0:g0 + hg].contiguous() for x in inp)
        whole = _device(a8, dev, inp, p, seed, offset)
        sub = _device(a8, dev, part, p, seed, offset, head0=g0)
        tags = prof_tags(lambda: _device(a8, dev, part, p, seed, offset, head0=g0))
        assert (NEW <= tags) == ((hg, d) in HD), tags
        cut = {k: v[:, g0:g0 + hg] for k, v in whole.items()}
        _compare(sub, cut, F32, p, "head0=%d hg=%d " % (g0, hg), factor=2)
        has = torch.bincount(g.src, minlength=g.n_src) > 0          # (rows without edges: (0, 0) fused, (-1e9, 0) composed)
        _compare(dict(stats=sub["stats"].cpu()[has]), dict(stats=cut["stats"].cpu()[has]), F32, 0.0, "stats ", factor=2,
                 keys=("stats",))
        _compare(sub, _reference(g, part, p, seed, offset, head0=g0), F32, p, "head0=%d hg=%d vs reference " % (g0, hg))
        # the decisions themselves
        ones = (torch.zeros_like(inp[0]), torch.zeros_like(inp[1]), torch.ones_like(inp[2]), torch.zeros_like(inp[3]),
                torch.ones_like(inp[4]))
        k_whole = _kept(_device(a8, dev, ones, p, seed, offset), g, d, p)
        k_sub = _kept(_device(a8, dev, tuple(x[:, g0:g0 + hg].contiguous() for x in ones), p, seed, offset, head0=g0), g, d, p)
        assert torch.equal(k_sub, k_whole[:, g0:g0 + hg])
        mult = A.head_multipliers(g.src.numpy(), g.dst.numpy(), 0, h, p, seed, offset)
        assert torch.equal(k_whole, mult > 0)


# ---- 8. knobs ------------------------------------------------------------------------------------------------------------------
def test_knobs(dev):
    """attn_rows = 0 (what existing tests set to get the composed path) and attn_heads = 0 keep the several-head form
    away.  Default knobs: on this graph (E = 2300 edges or so, 637 nodes) auto chooses the COMPOSED path for both shapes --
    the rule's first condition, (144 + 36 h) E > 32 h d (n_q + n_k), fails: the streams avoided do not pay for packing
    the operand tables (4 x 16: 0.66 M against 1.3 M; 8 x 32: 1.0 M against 5.2 M)."""
    g = _graph()
    a8 = _dev8(g.csr_args(), dev)
    try:
        for h, d in ((4, 16), (8, 32)):
            inp = _inputs(g, h, d, F32, seed=d)
            want = _reference(g, inp, *DROP)
            for knobs in (dict(attn_heads=1, attn_rows=0), dict(attn_heads=0), dict()):
                _lib.tune_reset()
                for k, v in knobs.items():
                    _lib.tune(k, v)
                _lib.clear_plan_cache()
                if not knobs:
                    assert (144 + 36 * h) * g.n_edges <= 32 * h * d * (g.n_src + g.n_dst)
                tags = prof_tags(lambda: _device(a8, dev, inp, *DROP))
                assert not (NEW & tags) and "attn_bias_add" in tags, (knobs, tags)
                Q, K = inp[0].to(dev), inp[1].to(dev)
                assert ops.attention_backward_is_fused(*a8, Q, K) is False
                _compare(_device(a8, dev, inp, *DROP), want, F32, DROP[0], "%s " % knobs)
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()


# ---- 9. the autograd classes ---------------------------------------------------------------------------------------------------
def _counting(monkeypatch, names):
    calls = {n: [] for n in names}
    for n in names:
        real = getattr(ops, n)
        monkeypatch.setattr(ops, n, lambda *a, _n=n, _real=real: (calls[_n].append(a), _real(*a))[1])
    return calls


@pytest.mark.parametrize("h,d", [(8, 32), (4, 16)])
def test_autograd_classes_make_one_call(dev, heads_on, h, d, monkeypatch):
    """FusedAttention, FusedAttentionDropout and FusedAttentionBias with attn_heads = 1: ONE attention_*_forward and one
    backward call for all heads (no head groups), results equal to the composed step and to the reference; b.grad has
    b's shape; b without a gradient asks the backward for no db."""
    g = random_graph(300, 300, 2700, seed=3 + h, chunk_size=8, zero_rows=0.2, hub=150)   # (square: the composed steps'
    gd = g.to(dev)                                                                        # SpMM returns zeros_like(V))
    inp = _inputs(g, h, d, F32, seed=5)
    Qc, Kc, Vc, bc, dOc = inp
    assert functions._head_group(h, d, g.n_edges, 300) in (1, 2, 4, 8)
    names = ("attention_forward", "attention_dropout_forward", "attention_bias_forward", "attention_backward",
             "attention_dropout_backward", "attention_bias_backward")
    calls = _counting(monkeypatch, names)

    def leaves():
        return tuple(x.to(dev).clone().requires_grad_(True) for x in (Qc, Kc, Vc))

    def grads(o, q, k, v):
        torch.cuda.synchronize()
        return dict(o=o.detach(), dQ=q.grad, dK=k.grad, dV=v.grad)

    keys = ("o", "dQ", "dK", "dV")
    # FusedAttention
    q, k, v = leaves()
    fused = grads(functions.fused_attention_step(gd, q, k, v, dOc.to(dev)), q, k, v)
    assert len(calls["attention_forward"]) == 1 and len(calls["attention_backward"]) == 1, {n: len(c) for n, c in calls.items()}
    want = A.reference_step(g.src, g.dst, g.n_src, Qc, Kc, Vc, dOc, 0.0, 0)
    q, k, v = leaves()
    composed = grads(functions.attention_step(gd, q, k, v, dOc.to(dev))[-1], q, k, v)
    _compare(fused, want, F32, 0.0, "FusedAttention ", keys=keys)
    _compare(fused, composed, F32, 0.0, "FusedAttention vs composed ", factor=2, keys=keys)
    # FusedAttentionDropout
    p, seed, offset = DROP
    q, k, v = leaves()
    fused = grads(functions.fused_attention_dropout_step(gd, q, k, v, dOc.to(dev), p, seed, offset), q, k, v)
    assert len(calls["attention_dropout_forward"]) == 1 and len(calls["attention_dropout_backward"]) == 1
    assert calls["attention_dropout_forward"][0][-1] == 0          # head0
    want = A.reference_step(g.src, g.dst, g.n_src, Qc, Kc, Vc, dOc, p, seed, offset)
    q, k, v = leaves()
    composed = grads(functions.attention_dropout_step(gd, q, k, v, dOc.to(dev), p, seed, offset)[-1], q, k, v)
    _compare(fused, want, F32, p, "FusedAttentionDropout ", keys=keys)
    _compare(fused, composed, F32, p, "FusedAttentionDropout vs composed ", factor=2, keys=keys)
    # FusedAttentionBias
    for drop in (NONE, DROP):
        n_f, n_b = len(calls["attention_bias_forward"]), len(calls["attention_bias_backward"])
        fused = _class_step(gd, inp, dev, drop)
        assert len(calls["attention_bias_forward"]) == n_f + 1 and len(calls["attention_bias_backward"]) == n_b + 1
        assert fused["db"].shape == bc.shape and calls["attention_bias_backward"][-1][-1] is True
        want = _reference(g, inp, *drop)
        composed = _class_step(gd, inp, dev, drop, functions.attention_bias_step)
        _compare(fused, want, F32, drop[0], "FusedAttentionBias p=%g " % drop[0])
        _compare(fused, composed, F32, drop[0], "FusedAttentionBias vs composed p=%g " % drop[0], factor=2)
    nodb = _class_step(gd, inp, dev, DROP, b_grad=False)
    assert nodb["db"] is None and calls["attention_bias_backward"][-1][-1] is False
    _compare(nodb, fused, F32, DROP[0], "b without grad ", factor=2, keys=keys)
    # and the passes were the several-head ones
    tags = prof_tags(lambda: _class_step(gd, inp, dev, DROP))
    assert NEW <= tags and not (COMPOSED & tags), tags


# ---- 10. HIP-graph replay ----------------------------------------------------------------------------------------------------------
def test_several_head_bias_step_replays_from_a_hip_graph(dev, heads_on):
    """One capture of forward and backward with prepared plans, replayed twice with new values in b (the capture rules
    of test_fused_bias_step_replays_from_a_hip_graph)."""
    import gc
    h, d, n = 4, 16, 1500
    g = random_graph(n, n, 15000, seed=3, chunk_size=32, hub=900).to(dev)
    gen = torch.Generator(device=dev).manual_seed(4)
    Q, K, V, dO = (torch.randn(n, h, d, device=dev, generator=gen) / 4 for _ in range(4))
    bs = [torch.randn(g.n_edges, h, device=dev, generator=gen) for _ in range(3)]
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
    b = bs[0].clone().requires_grad_(True)
    # nothing that earlier tests left behind (tracebacks holding device tensors and plans) may be finalised while the
    # stream is being captured: freeing a plan synchronises the device
    gc.collect()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        functions.fused_attention_bias_step(g, q, k, v, b, dO, *DROP)
    torch.cuda.current_stream().wait_stream(side)
    q.grad = k.grad = v.grad = b.grad = None
    graph = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            o = functions.fused_attention_bias_step(g, q, k, v, b, dO, *DROP)
    finally:
        gc.enable()
    p = DROP[0]
    for new in bs[1:]:
        with torch.no_grad():
            b.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        eager = _class_step(g, (Q, K, V, new, dO), dev, DROP)
        torch.testing.assert_close(o.detach(), eager["o"], rtol=1e-5, atol=1e-6 / (1 - p))
        for key, got in (("dQ", q.grad), ("dK", k.grad), ("dV", v.grad), ("db", b.grad)):
            torch.testing.assert_close(got, eager[key], rtol=1e-4, atol=1e-5 / (1 - p))
    assert NEW <= prof_tags(lambda: _class_step(g, (Q, K, V, bs[0], dO), dev, DROP))


# ---- 11. memory ----------------------------------------------------------------------------------------------------------------------
def test_several_head_bias_step_holds_nothing_edge_sized_but_db(dev):
    """N = 20000, E = 8 M, 8 x 32 (the graph of test_fused_head_groups_hold_no_e_by_h_tensor): the peak the several-head
    bias step adds over what is allocated before it is at most db, the node-sized results (o, stats, dQ, dK, dV), the
    two workspaces as the queries report them and 8 MB of allocator rounding -- and that bound is below db plus ONE
    further (E, h) array, so nothing else edge-sized can exist.  The head-group step (attn_heads = 0) adds more."""
    import ctypes
    N, E, h, d = 20000, 8_000_000, 8, 32
    g = graphs.chung_lu_graph(N, E, alpha=0.5, seed=3, device=dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    Q, K, V, dO = (torch.randn(N, h, d, device=dev, generator=gen) / 8 for _ in range(4))
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
    b = torch.randn(E, h, device=dev, generator=gen).requires_grad_(True)

    def step():
        q.grad = k.grad = v.grad = b.grad = None
        o = functions.fused_attention_bias_step(g, q, k, v, b, dO)
        return o

    def peak():
        for _ in range(2):
            step()
        q.grad = k.grad = v.grad = b.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    def query(backward, with_db):
        out = ctypes.c_int64(-1)
        a8 = g.csr_args()
        plan_r = _lib.get_plan(a8[0], a8[1], a8[2], a8[3], N)
        plan_c = _lib.get_plan(a8[4], a8[5], a8[6], a8[7], N)
        _lib.check(_lib.lib().graphop_attention_bias_workspace_bytes(
            0, backward, E, N, N, h, d, plan_r.handle, plan_c.handle, _lib.stream_of(Q), with_db, ctypes.byref(out)))
        return out.value

    try:
        _lib.tune("attn_heads", 1); _lib.clear_plan_cache()
        p_heads = peak()
        edge = E * h * 4
        node = N * h * d * 4
        bound = edge + 4 * node + N * h * 2 * 4 + query(0, 1) + query(1, 1) + 8 * 2 ** 20
        print("several-head bias step adds %.1f MB, bound %.1f MB, db %.1f MB" % (p_heads / 1e6, bound / 1e6, edge / 1e6))
        assert bound < 2 * edge, (bound, edge)
        assert p_heads <= bound, (p_heads, bound)
        heads = dict(o=step().detach().clone(), dQ=q.grad.clone(), db=b.grad.clone())
        _lib.tune("attn_heads", 0); _lib.clear_plan_cache()
        p_groups = peak()
        print("head-group bias step adds %.1f MB" % (p_groups / 1e6))
        assert p_groups > p_heads, (p_groups, p_heads)
        groups = dict(o=step().detach(), dQ=q.grad, db=b.grad)
        for key in heads:
            torch.testing.assert_close(heads[key], groups[key], rtol=2e-4, atol=2e-5)
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()
