"""GPU tier of the attention dropout of the fused dot-product attention step: graphop.attention_dropout_forward /
_backward, functions.FusedAttentionDropout and the two dropout steps against the float64 CPU statement of the definition
(tests/attention_dropout_reference.py), against each other and against the undropped op at p = 0.  Paths are forced
with the tuning knobs and asserted through the profile tags, as tests/test_fused_attention.py does.

Tolerances are that file's (fp32 rtol 1e-4 / atol 1e-5, fp64 1e-10 / 1e-12) with atol times 1 / (1 - p): every term of
every sum is scaled by it.  Two fp32 results compared with each other get twice that."""
import pytest
import torch

import attention_dropout_reference as A
import dropout_reference as R
from custom_op_benchmark_amd import _lib, functions, graphop as ops, graphs
from test_fused_attention import TOL, force_fwd_walk, force_sweep, prof_tags, shuffled_chunk_arrays  # noqa: F401
from util import random_graph

pytestmark = pytest.mark.gpu

KEYS = ("o", "dQ", "dK", "dV")
DROP = (0.6, 1234567890123, 7)


def _inputs(g, h, d, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    shape = (lambda n: (n, d) if h == 1 else (n, h, d))
    return tuple(torch.randn(*shape(n), generator=gen, dtype=torch.float64).to(dtype) / d ** 0.5
                 for n in (g.n_src, g.n_dst, g.n_dst, g.n_src))


def _reference(g, inp, p, seed, offset, head0=0):
    return A.reference_step(g.src, g.dst, g.n_src, *inp, p, seed, offset, head0)


def _device(a8, dev, inp, p, seed, offset, head0=0):
    Q, K, V, dO = (x.to(dev) for x in inp)
    o, stats = ops.attention_dropout_forward(*a8[:4], Q, K, V, p, seed, offset, head0)
    dQ, dK, dV = ops.attention_dropout_backward(*a8, Q, K, V, o, stats, dO, p, seed, offset, head0)
    torch.cuda.synchronize()
    return dict(o=o, dQ=dQ, dK=dK, dV=dV, stats=stats)


def _compare(got, want, dtype, p, what="", factor=1, keys=KEYS):
    tol = TOL[dtype]
    for k in keys:
        x, y = got[k], want[k]
        assert x.dtype == dtype and x.shape == y.shape, (what, k, x.shape, y.shape)
        torch.testing.assert_close(x.cpu().double(), y.cpu().double().reshape(x.shape), rtol=factor * tol["rtol"],
                                   atol=factor * tol["atol"] / (1 - p), msg=lambda m: "%s%s: %s" % (what, k, m))


def _seed_with_a_fully_dropped_row(g, h, p):
    """a seed at which the reference itself has a non-empty row all of whose edges are dropped (for some head)"""
    for seed in range(64):
        gone = R.fully_dropped_rows(g.src, g.dst, g.n_src, h, p, seed, 3)
        if gone.any():
            return seed, gone
    raise AssertionError("no seed below 64 drops a whole row")


def _tags_of(fn):
    tags = prof_tags(fn)
    return tags, {"attn_rows_row", "attn_rows_col", "attn_bwd_row", "attn_bwd_col", "attn_fwd"} & tags


# ---- 1. the composed paths against the float64 reference ------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h,d", [(1, 16), (2, 8), (5, 12), (8, 32)])
def test_composed_paths_match_the_float64_reference(dev, h, d, dtype):
    """Rectangular graph with empty rows and a hub row of parallel edges, chunk lists in order and shuffled (the
    plan-less softmax path); at p = 0.6 the seed is one at which a non-empty row loses every edge."""
    g = random_graph(90, 131, 1500, seed=5, chunk_size=8, zero_rows=0.2, hub=200)
    pairs = torch.stack([g.src, g.dst], 1)
    assert torch.unique(pairs, dim=0).size(0) < g.n_edges and g.n_src != g.n_dst          # parallel edges, rectangular
    assert (torch.bincount(g.src, minlength=g.n_src) == 0).any()                            # an empty row
    inp = _inputs(g, h, d, dtype, seed=h * 100 + d)
    layouts = (tuple(t.to(dev) for t in g.csr_args()), tuple(t.to(dev) for t in shuffled_chunk_arrays(g, seed=2)))
    _lib.tune("attn_rows", 0); _lib.clear_plan_cache()          # (fp32, h = 1, d = 16 would take the chunk-driver passes)
    try:
        for p in (0.1, 0.6):
            seed, gone = _seed_with_a_fully_dropped_row(g, h, p) if p == 0.6 else (1234567890123, None)
            want = _reference(g, inp, p, seed, 3)
            for which, a8 in enumerate(layouts):
                got = _device(a8, dev, inp, p, seed, 3)
                _compare(got, want, dtype, p, "h=%d d=%d p=%g layout %d " % (h, d, p, which))
                has = torch.bincount(g.src, minlength=g.n_src) > 0          # (rows without edges: see test_fused_forward_stats)
                _compare(dict(stats=got["stats"].cpu().reshape(g.n_src, h, 2)[has]), dict(stats=want["stats"][has]), dtype,
                         0.0, "stats ", keys=("stats",))
                if gone is not None:
                    assert gone.any()
                    o3, dq3 = (got[k].cpu().reshape(g.n_src, h, d) for k in ("o", "dQ"))
                    assert not o3[gone].any() and not dq3[gone].any()
        tags, fast = _tags_of(lambda: _device(layouts[0], dev, inp, 0.6, 1, 3))
        assert "attn_drop_apply" in tags and not fast, tags
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()


# ---- 2. the chunk-driver backward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 64, 256])
@pytest.mark.parametrize("chunk_size,rows_sorted", [(8, True), (8, False)])
def test_chunk_driver_backward_matches_the_reference(dev, d, chunk_size, rows_sorted):
    """attn_rows = 1: a hub row cut into many chunks, so that it is split over lane groups (the owned store, the shared
    flush and the atomics all run); with the chunk list shuffled no row is owned.  Row lengths are no multiples of the
    slot batch."""
    n = 64 if d >= 256 else 300
    g = random_graph(n, n + 37, 9 * n, seed=3 + d, chunk_size=chunk_size, zero_rows=0.2, hub=n // 2)
    inp = _inputs(g, 1, d, torch.float32, seed=4)
    a8 = g.csr_args() if rows_sorted else shuffled_chunk_arrays(g, seed=11)
    a8 = tuple(v.to(dev) for v in a8)
    p, seed, offset = DROP
    want = _reference(g, inp, p, seed, offset)
    _lib.tune("attn_rows", 1); _lib.clear_plan_cache()
    try:
        got = _device(a8, dev, inp, p, seed, offset)
        tags, _ = _tags_of(lambda: _device(a8, dev, inp, p, seed, offset))
        assert {"attn_rows_row", "attn_rows_col"} <= tags, tags
        _compare(got, want, torch.float32, p, "d=%d " % d)
        # a head other than 0: the Philox block and word of the one-head kernels (head0 = 6: block 1, word 2)
        got6 = _device(a8, dev, inp, p, seed, offset, head0=6)
        _compare(got6, _reference(g, inp, p, seed, offset, head0=6), torch.float32, p, "head0=6 d=%d " % d)
        assert not torch.equal(got6["o"], got["o"])
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()


# ---- 3. the window-owner backward --------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 64])
@pytest.mark.parametrize("staged", [0, 7])
def test_window_owner_backward_matches_the_reference(dev, force_sweep, d, staged):
    """force_sweep: windows of 4 KB (a few packed rows each, many windows per table), rows longer than vrow_t cut into
    pieces merged by atomics, ids per batch or staged through LDS (d = 64)."""
    _lib.tune("staged_ids", staged)
    g = random_graph(1500, 1541, 15000, seed=77 + d, chunk_size=32, zero_rows=0.15, hub=900)
    inp = _inputs(g, 1, d, torch.float32, seed=8)
    a8 = tuple(v.to(dev) for v in g.csr_args())
    p, seed, offset = DROP
    got = _device(a8, dev, inp, p, seed, offset, head0=3)
    tags, _ = _tags_of(lambda: _device(a8, dev, inp, p, seed, offset, head0=3))
    assert {"attn_bwd_row", "attn_bwd_col"} <= tags, tags
    _compare(got, _reference(g, inp, p, seed, offset, head0=3), torch.float32, p, "d=%d staged=%d " % (d, staged))


# ---- 4. the one-pass forward ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [8, 0])
def test_one_pass_forward_matches_the_reference(dev, force_fwd_walk, blocks):
    """The walk-style forward at a forced small geometry (rows cut by bin boundaries, whose piece records carry dropped
    and kept slots; a hub row over many bins; empty rows; padded last chunks): o and the statistics against the
    reference, the statistics against the undropped forward's."""
    _lib.tune("walk_blocks", blocks)
    g = random_graph(1500, 1541, 15000, seed=91 + blocks, chunk_size=32, zero_rows=0.15, hub=900)
    inp = _inputs(g, 1, 64, torch.float32, seed=12)
    gd = g.to(dev)
    a4 = (gd.row, gd.ptr_r, gd.eid_r, gd.indices_r)
    Q, K, V = (x.to(dev) for x in inp[:3])
    p, seed, offset = DROP
    _lib.profile_enable(True)
    try:
        o, stats = ops.attention_dropout_forward(*a4, Q, K, V, p, seed, offset, 5)
        torch.cuda.synchronize()
        prof = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    assert prof["attn_fwd"]["kernel"] == "k_attn_fwd_walk_f32<DROP>", prof
    assert not ({"sddmm_fwd", "softmax_fwd", "spmm_fwd", "attn_drop_apply"} & set(prof)), prof
    want = _reference(g, inp, p, seed, offset, head0=5)
    _compare(dict(o=o), want, torch.float32, p, keys=("o",))
    o0, stats0 = ops.attention_forward(*a4, Q, K, V)
    assert not torch.equal(o, o0)
    has = torch.bincount(g.src, minlength=g.n_src) > 0
    st, st0, ref = (x.cpu().reshape(-1, 2).double() for x in (stats, stats0, want["stats"]))
    for x in (st0, ref):          # (the bounds tests/test_fused_attention.py states for the undropped walk's statistics)
        torch.testing.assert_close(st[has, 0], x[has, 0], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(st[has, 1], x[has, 1], rtol=1e-4, atol=1e-7)
    assert float(st[~has].abs().max()) == 0.0
    gone = R.fully_dropped_rows(g.src, g.dst, g.n_src, 6, p, seed, offset)[:, 5]
    assert gone.any() and not o.cpu()[gone].any()


# ---- 5. fast, composed and generic agree ----------------------------------------------------------------------------------
def test_fast_composed_and_generic_paths_agree(dev):
    g = graphs.chung_lu_graph(20000, 200000, alpha=0.6, seed=0)
    inp = _inputs(g, 1, 64, torch.float32, seed=7)
    a8 = tuple(v.to(dev) for v in g.csr_args())
    p, seed, offset = DROP
    out = {}
    try:
        for name, knobs in (("fast", dict(sweep_min_kb=0, window_kb=64, sweep_min_granule=0)),
                            ("composed", dict(attn_fused=0)), ("generic", dict(force_generic=1))):
            _lib.tune_reset()
            for k, v in knobs.items():
                _lib.tune(k, v)
            _lib.clear_plan_cache()
            out[name] = _device(a8, dev, inp, p, seed, offset)
            tags, fast = _tags_of(lambda: _device(a8, dev, inp, p, seed, offset))
            if name == "fast":          # (the forward is the composed one here: only test 4 forces the one-pass form)
                assert {"attn_bwd_row", "attn_bwd_col"} <= tags, tags
            else:
                assert "attn_drop_apply" in tags and not fast, tags
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()
    for other in ("composed", "generic"):
        _compare(out["fast"], out[other], torch.float32, p, "fast vs %s " % other, factor=2)
    _compare(out["composed"], out["generic"], torch.float32, p, "composed vs generic ", factor=2)


# ---- 6. p = 0 is the undropped op, bit for bit -------------------------------------------------------------------------------
def _unsplit_graph(seed, n=300):
    """No row and no column is split over chunks: nothing is summed by atomics, results are repeatable bit for bit."""
    g = random_graph(n, n, 10 * n, seed=seed, chunk_size=32)
    assert torch.bincount(g.src).max() <= 32 and torch.bincount(g.dst).max() <= 32
    return g


def _p_zero_equals_undropped(g, dev, h, d, dtype, want_tags):
    a8 = tuple(v.to(dev) for v in g.csr_args())
    Q, K, V, dO = (x.to(dev) for x in _inputs(g, h, d, dtype, seed=h + d))

    def plain():
        o, stats = ops.attention_forward(*a8[:4], Q, K, V)
        return [o, stats] + ops.attention_backward(*a8, Q, K, V, o, stats, dO)

    def dropped():
        o, stats = ops.attention_dropout_forward(*a8[:4], Q, K, V, 0.0, 77, 5, 2)
        return [o, stats] + ops.attention_dropout_backward(*a8, Q, K, V, o, stats, dO, 0.0, 77, 5, 2)

    _lib.profile_enable(True)
    try:
        dropped()
        torch.cuda.synchronize()
        prof = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    tags = set(prof)
    assert want_tags <= tags and "attn_drop_apply" not in tags, tags
    assert not [r["kernel"] for r in prof.values() if "DROP" in r["kernel"]], prof      # the undropped instantiations
    for x, y in zip(plain(), dropped()):
        assert torch.equal(x, y), (h, d, dtype, sorted(tags))


def test_p_zero_is_bit_identical_composed_and_chunk_driver(dev):
    g = _unsplit_graph(3)
    try:
        _lib.tune("attn_rows", 0); _lib.clear_plan_cache()
        for h, d, dtype in ((1, 16, torch.float32), (2, 8, torch.float32), (1, 8, torch.float64)):
            _p_zero_equals_undropped(g, dev, h, d, dtype, {"sddmm_fwd"})
        _lib.tune("attn_rows", 1); _lib.clear_plan_cache()
        for d in (16, 64):
            _p_zero_equals_undropped(g, dev, 1, d, torch.float32, {"attn_rows_row", "attn_rows_col"})
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()


def test_p_zero_is_bit_identical_window_owner(dev, force_sweep):
    """Complete bipartite blocks of 8 rows x 8 columns, each inside one column window of either table (windows of 4 KB
    hold 8 packed rows of d = 64; the blocks start at multiples of 32) and shorter than a piece: every row is flushed
    exactly once, so nothing depends on the order of the atomics and the results are repeatable bit for bit."""
    _p_zero_equals_undropped(_block_graph(300), dev, 1, 64, torch.float32, {"attn_bwd_row", "attn_bwd_col"})


def _block_graph(n, chunk_size=32):
    """Complete bipartite blocks of 8 rows x 8 columns starting at the multiples of 32 below n: every row and every column
    has 8 edges, all inside one column window of either table at any window size from 8 rows up."""
    base = torch.arange(0, n - 8, 32)
    rows = (base[:, None] + torch.arange(8)[None, :]).reshape(-1)
    src = rows.repeat_interleave(8)
    dst = (base[:, None, None] + torch.arange(8)[None, None, :]).expand(-1, 8, -1).reshape(-1)
    return graphs.graph_from_coo(src, dst, n, n, chunk_size)


def test_p_zero_is_bit_identical_one_pass_forward(dev, force_fwd_walk):
    """Rows of 8 slots in bins of some 90 (walk_blocks = 8): a row that a bin boundary cuts leaves two pieces, and two pieces
    added into a zero-filled row give the same bits in either order, so the one-pass forward is repeatable here and p = 0
    can be held to torch.equal.  The profile names the instantiation: p = 0 runs the undropped one."""
    _lib.tune("walk_blocks", 8)
    g = _block_graph(6000).to(dev)          # (two 1.5 MB tables in windows of 8 KB: 512 windows, the most the walk takes)
    a4 = (g.row, g.ptr_r, g.eid_r, g.indices_r)
    Q, K, V, _ = (x.to(dev) for x in _inputs(g, 1, 64, torch.float32, seed=1))

    def records(fn):
        _lib.profile_enable(True)
        try:
            out = fn()
            torch.cuda.synchronize()
            return out, {t: r["kernel"] for t, r in _lib.profile_read().items()}
        finally:
            _lib.profile_enable(False)

    plain, k0 = records(lambda: ops.attention_forward(*a4, Q, K, V))
    dropped, k1 = records(lambda: ops.attention_dropout_forward(*a4, Q, K, V, 0.0, 77, 5, 2))
    assert k0 == k1 and k0["attn_fwd"] == "k_attn_fwd_walk_f32", (k0, k1)
    _, k2 = records(lambda: ops.attention_dropout_forward(*a4, Q, K, V, 0.5, 77, 5, 2))
    assert k2["attn_fwd"] == "k_attn_fwd_walk_f32<DROP>", k2
    for x, y in zip(plain, dropped):
        assert torch.equal(x, y)
    # ... and the autograd class at p = 0 is FusedAttention
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
    o0 = functions.FusedAttention.apply(*g.csr_args(), q, k, v)
    o1 = functions.FusedAttentionDropout.apply(*g.csr_args(), q, k, v, 0.0, 1, 2)
    assert torch.equal(o0, o1)
    assert type(o1.grad_fn).__name__.startswith("FusedAttentionDropout")


# ---- 7. repeatability ------------------------------------------------------------------------------------------------------
def test_same_seed_and_offset_repeat_bit_for_bit_and_the_offset_matters(dev):
    g = _unsplit_graph(3)
    a8 = tuple(v.to(dev) for v in g.csr_args())
    try:
        for h, d, rows in ((1, 64, 1), (1, 16, 1), (2, 8, 0), (8, 4, 0)):
            _lib.tune("attn_rows", rows); _lib.clear_plan_cache()
            inp = _inputs(g, h, d, torch.float32, seed=h)
            run = lambda seed, off: _device(a8, dev, inp, 0.5, seed, off)
            a, b, c, e = run(11, 0), run(11, 0), run(11, 1), run(12, 0)
            for k in KEYS + ("stats",):
                assert torch.equal(a[k], b[k]), (h, d, k)
            assert not torch.equal(a["o"], c["o"]) and not torch.equal(a["o"], e["o"])
            assert torch.equal(a["stats"], c["stats"])
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()
    # the autograd class: seed=None draws from torch's default CPU generator
    Q, K, V, _ = (x.to(dev) for x in _inputs(g, 1, 16, torch.float32, seed=2))
    outs = []
    for _ in range(2):
        torch.manual_seed(5)
        outs.append(functions.FusedAttentionDropout.apply(*a8, Q, K, V, 0.5, None, 0))
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[0], functions.FusedAttentionDropout.apply(*a8, Q, K, V, 0.5, None, 0))


# ---- 8. head groups: head0 on the device ----------------------------------------------------------------------------------
def _class_step(g, inp, dev, drop):
    Q, K, V = (x.to(dev).clone().requires_grad_(True) for x in inp[:3])
    o = functions.FusedAttentionDropout.apply(*g.csr_args(), Q, K, V, *drop)
    o.backward(inp[3].to(dev))
    torch.cuda.synchronize()
    return dict(o=o.detach(), dQ=Q.grad, dK=K.grad, dV=V.grad)


@pytest.mark.parametrize("h,d,hg", [(8, 32, 2), (4, 16, 2), (8, 32, 1)])
def test_head_groups_make_the_decisions_of_one_call(dev, force_sweep, h, d, hg, monkeypatch):
    """FusedAttentionDropout in head groups (the group size set as test_fused_head_groups_vs_oracle sets it): grouped
    equals ungrouped equals the reference.  Groups of 2 start at heads that are no multiples of four; groups of one head
    of d = 32 run the fused one-head kernels with head0 = 0 .. 7."""
    g = random_graph(700, 941, 14000, seed=3 + h + d, chunk_size=32, zero_rows=0.1, hub=900)
    inp = _inputs(g, h, d, torch.float32, seed=5)
    gd = g.to(dev)
    want = _reference(g, inp, *DROP)
    monkeypatch.setattr(functions, "_head_group", lambda h_, d_, *sizes: hg)
    grouped = _class_step(gd, inp, dev, DROP)
    tags, fast = _tags_of(lambda: _class_step(gd, inp, dev, DROP))
    if hg == 1:          # (d = 32: the backward of every head is fused, the forward composed)
        assert {"attn_bwd_row", "attn_bwd_col"} <= tags, tags
    else:
        assert "attn_drop_apply" in tags and not fast, tags
    monkeypatch.setattr(functions, "_head_group", lambda h_, d_, *sizes: h_)
    ungrouped = _class_step(gd, inp, dev, DROP)
    _compare(grouped, want, torch.float32, DROP[0], "grouped ")
    _compare(ungrouped, want, torch.float32, DROP[0], "ungrouped ")
    _compare(grouped, ungrouped, torch.float32, DROP[0], "grouped vs ungrouped ", factor=2)


# ---- 9. gradcheck -------------------------------------------------------------------------------------------------------------
def test_gradcheck_fp64(dev):
    g = random_graph(12, 10, 50, seed=4, chunk_size=3, hub=8).to(dev)
    for h, d in ((1, 3), (2, 4), (5, 2)):
        inputs = tuple(x.to(dev).requires_grad_(True) for x in _inputs(g, h, d, torch.float64, seed=h)[:3])
        assert torch.autograd.gradcheck(
            lambda q, k, v: functions.FusedAttentionDropout.apply(*g.csr_args(), q, k, v, 0.5, 42, 3), inputs,
            nondet_tol=1e-12)   # (split rows are summed by float atomics: the order of the adds may differ)


# ---- 10. the bindings ------------------------------------------------------------------------------------------------------
def test_bindings_agree_and_refuse_bad_arguments(dev):
    """The ctypes binding and the compiled extension run the same entry points.  (torch.ops.graphop holds the ops of
    graphop._SCHEMAS only; the dropout form of the fused step is not among them.)"""
    ext = ops.cpp_ext
    assert ext is not None, "graphop_cpp.so not built (run __graft_entry__.build())"
    g = random_graph(500, 400, 8000, seed=6, chunk_size=32, hub=900).to(dev)
    a8 = g.csr_args()
    dr = (0.6, 2 ** 63 - 1, 2 ** 32 - 1, 5)
    for h, d in ((1, 64), (1, 16), (4, 16), (3, 8)):
        Q, K, V, dO = (x.to(dev) for x in _inputs(g, h, d, torch.float32, seed=h))
        f0 = ops.attention_dropout_forward(*a8[:4], Q, K, V, *dr)
        f1 = ext.attention_dropout_forward(*a8[:4], Q, K, V, p=dr[0], seed=dr[1], offset=dr[2], head0=dr[3])
        for u, v in zip(f0, f1):   # (rows split over lane groups are summed by atomics, in any order)
            torch.testing.assert_close(u, v, rtol=1e-5, atol=1e-6 / (1 - dr[0]))
        b0 = ops.attention_dropout_backward(*a8, Q, K, V, *f0, dO, *dr)
        b1 = ext.attention_dropout_backward(*a8, Q, K, V, *f0, dO, *dr)
        for u, v in zip(b0, b1):
            torch.testing.assert_close(u, v, rtol=1e-4, atol=1e-5 / (1 - dr[0]))
    for kw, msg in ((dict(p=1.0), r"p must be in \[0, 1\)"), (dict(p=-0.5), r"p must be in \[0, 1\)"),
                    (dict(p=0.5, seed=2 ** 63), "seed"), (dict(p=0.5, seed=-1), "seed"),
                    (dict(p=0.5, offset=2 ** 32), "offset"), (dict(p=0.5, offset=-1), "offset")):
        with pytest.raises(RuntimeError, match=msg):
            ops.attention_dropout_forward(*a8[:4], Q, K, V, **kw)
        with pytest.raises(RuntimeError, match=msg):
            ops.attention_dropout_backward(*a8, Q, K, V, *f0, dO, **kw)
        with pytest.raises(RuntimeError, match=msg):
            functions.FusedAttentionDropout.apply(*a8, Q, K, V, kw["p"], kw.get("seed", 0), kw.get("offset", 0))
        if kw.get("seed", 0) < 2 ** 63:          # (pybind refuses an int beyond int64 with a TypeError of its own)
            with pytest.raises(RuntimeError, match=msg):
                ext.attention_dropout_forward(*a8[:4], Q, K, V, **kw)
    with pytest.raises(RuntimeError, match="o, dO must match Q"):
        ops.attention_dropout_backward(*a8, Q, K, V, *f0, dO[:10], 0.5)
    with pytest.raises(RuntimeError, match="Q must be a CUDA tensor"):
        ops.attention_dropout_forward(*a8[:4], Q.cpu(), K, V, 0.5)


# ---- 11. HIP-graph replay ----------------------------------------------------------------------------------------------------
def test_fused_dropout_step_replays_from_a_hip_graph(dev, force_sweep):
    import gc
    g = random_graph(1500, 1500, 15000, seed=3, chunk_size=32, hub=900).to(dev)
    gen = torch.Generator(device=dev).manual_seed(4)
    Q, K, V, dO = (torch.randn(1500, 64, device=dev, generator=gen) / 8 for _ in range(4))
    eager = _class_step(g, (Q, K, V, dO), dev, DROP)
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
    # nothing that earlier tests left behind (tracebacks holding device tensors and plans) may be finalised while the
    # stream is being captured: freeing a plan synchronises the device
    gc.collect()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        functions.fused_attention_dropout_step(g, q, k, v, dO, *DROP)
    torch.cuda.current_stream().wait_stream(side)
    q.grad = k.grad = v.grad = None
    graph = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            o = functions.fused_attention_dropout_step(g, q, k, v, dO, *DROP)
    finally:
        gc.enable()
    graph.replay()
    torch.cuda.synchronize()
    p = DROP[0]
    torch.testing.assert_close(o.detach(), eager["o"], rtol=1e-5, atol=1e-6 / (1 - p))
    for key, got in (("dQ", q.grad), ("dK", k.grad), ("dV", v.grad)):
        torch.testing.assert_close(got, eager[key], rtol=1e-4, atol=1e-5 / (1 - p))


# ---- 12. no edge-sized tensor between forward and backward -----------------------------------------------------------------
def test_fused_dropout_step_keeps_no_edge_sized_tensor(dev):
    """h = 1, d = 64: what the fused dropout forward leaves allocated for its backward is below one (E,) fp32 tensor (it
    is o and the row statistics); the composed dropout step holds more than three (s, a, the mask, a * mask)."""
    g = graphs.chung_lu_graph(20000, 4_000_000, alpha=0.5, seed=0, device=dev)
    one = g.n_edges * 4
    Q, K, V, _ = (x.to(dev) for x in _inputs(g, 1, 64, torch.float32, seed=1))
    a8 = g.csr_args()

    def held(forward):
        leaves = [x.clone().requires_grad_(True) for x in (Q, K, V)]
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        o = forward(*leaves)
        torch.cuda.synchronize()
        kept = torch.cuda.memory_allocated() - base
        o.backward(torch.ones_like(o))
        torch.cuda.synchronize()
        return kept

    def fused(q, k, v):
        return functions.FusedAttentionDropout.apply(*a8, q, k, v, *DROP)

    def composed(q, k, v):
        a = functions.SparseSoftmax.apply(g.row, g.ptr_r, g.eid_r, functions.MaskedMMCSR.apply(*a8, q, k))
        mask = ops.edge_dropout_mask(g.row, g.ptr_r, g.eid_r, g.indices_r, 1, *DROP, a.dtype)
        return functions.VectorSPMM.apply(*a8, a * mask, v)

    held(fused)                       # plans of both orientations are built (and cached) here
    kept_fused, kept_composed = held(fused), held(composed)
    print("held between forward and backward: fused %d, composed %d, one (E,) tensor %d" % (kept_fused, kept_composed, one))
    assert kept_fused < one, (kept_fused, one)
    assert kept_composed > 3 * one, (kept_composed, one)
