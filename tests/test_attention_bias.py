"""GPU tier of the per-edge score bias of the fused dot-product attention step: graphop.attention_bias_forward /
_backward, functions.FusedAttentionBias and the two bias steps against the float64 CPU statement of the definition
(tests/attention_bias_reference.py), against each other and against the op without a bias at b = 0.  Paths are forced
with the tuning knobs and asserted through the profile tags, as tests/test_fused_attention.py does.

Tolerances are that file's (fp32 rtol 1e-4 / atol 1e-5, fp64 1e-10 / 1e-12) with atol times 1 / (1 - p): every term of
every sum is scaled by it.  Two fp32 results compared with each other get twice that.  Inputs: Q, K ~ randn / sqrt(d),
b ~ randn."""
import pytest
import torch

import attention_bias_reference as B
import gat_edge_reference as GE
from custom_op_benchmark_amd import _lib, functions, graphop as ops
from test_fused_attention import TOL, force_sweep, prof_tags, shuffled_chunk_arrays  # noqa: F401
from util import random_graph

pytestmark = pytest.mark.gpu

KEYS = ("o", "dQ", "dK", "dV", "db")
DROP = (0.6, 1234567890123, 7)
NONE = (0.0, 0, 0)
FAST_BWD = {"attn_bias_rows_row", "attn_bias_rows_col"}
FAST = FAST_BWD | {"attn_bias_fwd_rows", "attn_rows_row", "attn_rows_col", "attn_bwd_row", "attn_bwd_col", "attn_fwd"}


def _inputs(g, h, d, dtype, seed):
    """(Q, K, V, b, dO)"""
    gen = torch.Generator().manual_seed(seed)
    shape = (lambda n: (n, d) if h == 1 else (n, h, d))
    Q, K, V, dO = (torch.randn(*shape(n), generator=gen, dtype=torch.float64).to(dtype) / d ** 0.5
                   for n in (g.n_src, g.n_dst, g.n_dst, g.n_src))
    b = torch.randn(*((g.n_edges,) if h == 1 else (g.n_edges, h)), generator=gen, dtype=torch.float64).to(dtype)
    return Q, K, V, b, dO


def _reference(g, inp, p, seed, offset, head0=0, src=None, dst=None):
    return B.reference_step(g.src if src is None else src, g.dst if dst is None else dst, g.n_src, *inp, p, seed, offset,
                            head0)


def _device(a8, dev, inp, p, seed, offset, head0=0, need_db=True):
    Q, K, V, b, dO = (x.to(dev) for x in inp)
    o, stats = ops.attention_bias_forward(*a8[:4], Q, K, V, b, p, seed, offset, head0)
    dQ, dK, dV, db = ops.attention_bias_backward(*a8, Q, K, V, b, o, stats, dO, p, seed, offset, head0, need_db)
    torch.cuda.synchronize()
    return dict(o=o, dQ=dQ, dK=dK, dV=dV, db=db, stats=stats)


def _compare(got, want, dtype, p, what="", factor=1, keys=KEYS):
    tol = TOL[dtype]
    for k in keys:
        x, y = got[k], want[k]
        assert x.dtype == dtype and x.shape == y.reshape(x.shape).shape, (what, k, x.shape, y.shape)
        torch.testing.assert_close(x.cpu().double(), y.cpu().double().reshape(x.shape), rtol=factor * tol["rtol"],
                                   atol=factor * tol["atol"] / (1 - p), msg=lambda m: "%s%s: %s" % (what, k, m))


def _compare_stats(g, got, want, dtype, what="", empty_zero=False):
    """the statistics of the rows with edges against the reference's; empty_zero: rows without edges read (0, 0) (the
    fused forward; the plan-less softmax of the composed one leaves (-1e9, 0), see test_fused_forward_stats)"""
    h = want["stats"].size(1)
    has = torch.bincount(g.src, minlength=g.n_src) > 0
    st = got["stats"].cpu().reshape(g.n_src, h, 2)
    _compare(dict(stats=st[has]), dict(stats=want["stats"][has]), dtype, 0.0, what + "stats ", keys=("stats",))
    assert not empty_zero or not st[~has].any(), what


def _dev8(a8, dev):
    return tuple(t.to(dev) for t in a8)


# ---- 1. the composed paths against the float64 reference ------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("h,d", [(1, 16), (2, 8), (5, 12)])
def test_composed_paths_match_the_float64_reference(dev, h, d, dtype):
    """Rectangular graph with empty rows and a hub row of parallel edges, chunk lists in order and shuffled (the
    plan-less softmax path), without and with dropout."""
    g = random_graph(90, 131, 1500, seed=5, chunk_size=8, zero_rows=0.2, hub=200)
    assert torch.unique(torch.stack([g.src, g.dst], 1), dim=0).size(0) < g.n_edges and g.n_src != g.n_dst
    assert (torch.bincount(g.src, minlength=g.n_src) == 0).any()
    inp = _inputs(g, h, d, dtype, seed=h * 100 + d)
    layouts = (_dev8(g.csr_args(), dev), _dev8(shuffled_chunk_arrays(g, seed=2), dev))
    _lib.tune("attn_rows", 0); _lib.clear_plan_cache()          # (fp32, h = 1, d = 16 would take the chunk-driver passes)
    try:
        for p, seed, offset in (NONE, DROP):
            want = _reference(g, inp, p, seed, offset)
            for which, a8 in enumerate(layouts):
                what = "h=%d d=%d p=%g layout %d " % (h, d, p, which)
                got = _device(a8, dev, inp, p, seed, offset)
                _compare(got, want, dtype, p, what)
                _compare_stats(g, got, want, dtype, what)
                tags = prof_tags(lambda: _device(a8, dev, inp, p, seed, offset))
                assert "attn_bias_add" in tags and not (FAST & tags), tags
                assert ("attn_drop_apply" in tags) == (p > 0), tags
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()


# ---- 2. the chunk-driver backward ---------------------------------------------------------------------------------------
def _hub_graph(d, seed=3):
    n = 64 if d >= 256 else 300
    return random_graph(n, n + 37, 9 * n, seed=seed + d, chunk_size=8, zero_rows=0.2, hub=n // 2)


@pytest.mark.parametrize("d", [16, 64, 256])
@pytest.mark.parametrize("rows_sorted", [True, False])
def test_chunk_driver_backward_matches_the_reference(dev, d, rows_sorted):
    """attn_rows = 1: a hub row of n // 2 edges cut into chunks of 8, so that it is split over many lane groups (the owned
    store, the shared flush and the atomics all run); with the chunk list shuffled no row is owned.  Row lengths are no
    multiples of the slot batch.  need_db=False: the same dQ / dK / dV (rows that several lane groups share are summed by
    float atomics in any order, so the comparison on this graph is at the two-results tolerance; the bit-for-bit one is
    test_need_db_false_changes_no_other_bit) and an empty db."""
    g = _hub_graph(d)
    assert (torch.bincount(g.src) % 8 != 0).any() and torch.bincount(g.src).max() >= (64 if d >= 256 else 300) // 2
    inp = _inputs(g, 1, d, torch.float32, seed=4)
    a8 = _dev8(g.csr_args() if rows_sorted else shuffled_chunk_arrays(g, seed=11), dev)
    _lib.tune("attn_rows", 1); _lib.clear_plan_cache()
    try:
        for p, seed, offset in (NONE, DROP):
            want = _reference(g, inp, p, seed, offset)
            got = _device(a8, dev, inp, p, seed, offset)
            tags = prof_tags(lambda: _device(a8, dev, inp, p, seed, offset))
            assert FAST_BWD <= tags and ("attn_bias_fwd_rows" in tags) == rows_sorted, tags
            assert not ({"attn_rows_row", "attn_bwd_row", "attn_bias_add"} & tags) or not rows_sorted, tags
            _compare(got, want, torch.float32, p, "d=%d p=%g " % (d, p))
            _compare_stats(g, got, want, torch.float32, "d=%d p=%g " % (d, p))
            nodb = _device(a8, dev, inp, p, seed, offset, need_db=False)
            assert nodb["db"].numel() == 0 and nodb["db"].dtype == torch.float32
            _compare(nodb, got, torch.float32, p, "need_db=False ", factor=2, keys=("dQ", "dK", "dV"))
        # a head other than 0: the Philox block and word of the one-head kernels (head0 = 6: block 1, word 2)
        p, seed, offset = DROP
        got6 = _device(a8, dev, inp, p, seed, offset, head0=6)
        _compare(got6, _reference(g, inp, p, seed, offset, head0=6), torch.float32, p, "head0=6 d=%d " % d)
        assert not torch.equal(got6["o"], got["o"])
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()


@pytest.mark.parametrize("d", [16, 64])
@pytest.mark.parametrize("rows_sorted", [True, False])
def test_bias_is_addressed_by_edge_id_not_by_slot(dev, d, rows_sorted):
    """The edges renumbered by a random permutation (eid_r a permutation, eid_c consistent with it, the slots where they
    were): b and db follow the edge ids.  The plans do not say eid_identity, so both passes read their eid arrays."""
    g0 = _hub_graph(d, seed=9)
    g, src, dst = GE.permute_edge_ids(g0, 5)
    assert not torch.equal(g.eid_r, torch.arange(g.n_edges)) and torch.equal(src[g.eid_r], g0.src[g0.eid_r])
    inp = _inputs(g, 1, d, torch.float32, seed=6)
    a8 = _dev8(g.csr_args() if rows_sorted else shuffled_chunk_arrays(g, seed=13), dev)
    _lib.tune("attn_rows", 1); _lib.clear_plan_cache()
    try:
        for p, seed, offset in (NONE, DROP):
            got = _device(a8, dev, inp, p, seed, offset)
            _compare(got, _reference(g, inp, p, seed, offset, src=src, dst=dst), torch.float32, p, "permuted p=%g " % p)
        tags = prof_tags(lambda: _device(a8, dev, inp, *DROP))
        assert FAST_BWD <= tags and ("attn_bias_fwd_rows" in tags) == rows_sorted, tags
        # the same b read by slot instead would be another result: the identity numbering with this b differs
        other = _device(_dev8(g0.csr_args(), dev), dev, inp, *NONE)
        assert not torch.allclose(other["o"], _device(a8, dev, inp, *NONE)["o"], rtol=1e-3, atol=1e-4)
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()


def _unsplit_graph(seed, n=300):
    """No row and no column is split over chunks: nothing is summed by atomics, results are repeatable bit for bit."""
    g = random_graph(n, n, 10 * n, seed=seed, chunk_size=32)
    assert torch.bincount(g.src).max() <= 32 and torch.bincount(g.dst).max() <= 32
    return g


def test_need_db_false_changes_no_other_bit(dev):
    g = _unsplit_graph(3)
    a8 = _dev8(g.csr_args(), dev)
    try:
        for rows, h, d in ((1, 1, 16), (1, 1, 64), (0, 1, 16), (0, 3, 8)):
            _lib.tune("attn_rows", rows); _lib.clear_plan_cache()
            inp = _inputs(g, h, d, torch.float32, seed=d)
            for drop in (NONE, DROP):
                a, b = _device(a8, dev, inp, *drop), _device(a8, dev, inp, *drop, need_db=False)
                for k in ("o", "stats", "dQ", "dK", "dV"):
                    assert torch.equal(a[k], b[k]), (rows, h, d, drop, k)
                assert b["db"].numel() == 0 and a["db"].shape == inp[3].shape
            tags = prof_tags(lambda: _device(a8, dev, inp, *NONE, need_db=False))
            assert (FAST_BWD <= tags) == bool(rows), tags
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()


# ---- 3. the fused forward -------------------------------------------------------------------------------------------------
def _forward(a8, dev, inp, p, seed, offset, head0=0):
    Q, K, V, b, _ = (x.to(dev) for x in inp)
    o, stats = ops.attention_bias_forward(*a8[:4], Q, K, V, b, p, seed, offset, head0)
    torch.cuda.synchronize()
    return dict(o=o, stats=stats)


@pytest.mark.parametrize("d", [16, 64, 256])
def test_fused_forward_matches_the_reference(dev, d):
    """One lane group per chunk of 8 slots on these graphs: the hub row of n // 2 edges spans many groups, every group
    strictly inside it emits a single mid-row piece, its first group the flagged one; rows of one chunk are stored
    whole, rows of two chunks leave two pieces; rows without edges keep stats (0, 0) and o = 0.  With the chunk list
    shuffled the composed forward runs."""
    g = _hub_graph(d)
    hub = int(torch.bincount(g.src).argmax())
    assert int((g.row == hub).sum()) >= 3          # at least three lane groups at one chunk per group
    inp = _inputs(g, 1, d, torch.float32, seed=4)
    a8 = _dev8(g.csr_args(), dev)
    sh8 = _dev8(shuffled_chunk_arrays(g, seed=11), dev)
    for p, seed, offset in (NONE, DROP):
        want = _reference(g, inp, p, seed, offset, head0=5)
        got = _forward(a8, dev, inp, p, seed, offset, 5)
        tags = prof_tags(lambda: _forward(a8, dev, inp, p, seed, offset, 5))
        assert "attn_bias_fwd_rows" in tags and not ({"sddmm_fwd", "softmax_fwd", "spmm_fwd", "attn_bias_add"} & tags), tags
        _compare(got, want, torch.float32, p, "d=%d p=%g " % (d, p), keys=("o",))
        _compare_stats(g, got, want, torch.float32, "d=%d p=%g " % (d, p), empty_zero=True)
        assert not got["o"].cpu()[torch.bincount(g.src, minlength=g.n_src) == 0].any()
        got_s = _forward(sh8, dev, inp, p, seed, offset, 5)
        tags = prof_tags(lambda: _forward(sh8, dev, inp, p, seed, offset, 5))
        assert "attn_bias_fwd_rows" not in tags and "attn_bias_add" in tags, tags
        _compare(got_s, want, torch.float32, p, "shuffled d=%d p=%g " % (d, p), keys=("o",))
        _compare_stats(g, got_s, want, torch.float32, "shuffled ")
    try:          # the knob that forbids the chunk-driver forms forbids this one
        _lib.tune("attn_rows", 0); _lib.clear_plan_cache()
        assert "attn_bias_fwd_rows" not in prof_tags(lambda: _forward(a8, dev, inp, *NONE))
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()


# ---- 4. more than one chunk per lane group ------------------------------------------------------------------------------
def test_several_chunks_per_lane_group(dev):
    """d = 64 and chunks of one slot, enough of them that the launches' rule clamp(n_chunks / (n_cu * (256 / L) * 8), 1,
    16) gives cpg >= 2 on this device, and no multiple of cpg: the last group's run is short.  Rows of ~37 chunks over
    groups of cpg: most groups start inside one row and end inside another (first and last row both shared, two pieces),
    the rows between are stored whole."""
    L, d = 16, 64
    g = random_graph(3000, 3000, 110000, seed=17, chunk_size=1)
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    n_chunks = g.row.numel()
    cpg = min(16, max(1, n_chunks // (n_cu * (256 // L) * 8)))
    assert cpg >= 2 and n_chunks % cpg != 0, (n_chunks, n_cu, cpg)
    row, both = g.row.tolist(), 0
    for c0 in range(cpg, n_chunks - cpg, cpg):
        first, last = row[c0], row[c0 + cpg - 1]
        both += first != last and first == row[c0 - 1] and last == row[c0 + cpg]
    assert both > 0          # some group's first row and last row are both shared
    inp = _inputs(g, 1, d, torch.float32, seed=2)
    a8 = _dev8(g.csr_args(), dev)
    _lib.tune("attn_rows", 1); _lib.clear_plan_cache()
    try:
        got = _device(a8, dev, inp, *DROP)
        tags = prof_tags(lambda: _device(a8, dev, inp, *DROP))
        assert FAST_BWD | {"attn_bias_fwd_rows"} <= tags, tags
        want = _reference(g, inp, *DROP)
        _compare(got, want, torch.float32, DROP[0], "cpg=%d " % cpg)
        _compare_stats(g, got, want, torch.float32, "cpg=%d " % cpg, empty_zero=True)
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()


# ---- 5. window-shaped graphs take the chunk-driver form with the bias ---------------------------------------------------
def test_window_shaped_graphs_take_the_chunk_driver_bias_form(dev, force_sweep):
    g = random_graph(1500, 1541, 15000, seed=77, chunk_size=32, zero_rows=0.15, hub=900)
    inp = _inputs(g, 1, 64, torch.float32, seed=8)
    a8 = _dev8(g.csr_args(), dev)
    Q, K, V, b, dO = (x.to(dev) for x in inp)

    def plain():
        o, stats = ops.attention_forward(*a8[:4], Q, K, V)
        return ops.attention_backward(*a8, Q, K, V, o, stats, dO)

    assert {"attn_bwd_row", "attn_bwd_col"} <= prof_tags(plain)
    tags = prof_tags(lambda: _device(a8, dev, inp, *DROP))
    assert FAST_BWD <= tags and not ({"attn_bwd_row", "attn_bwd_col", "attn_bias_add"} & tags), tags
    _compare(_device(a8, dev, inp, *DROP), _reference(g, inp, *DROP), torch.float32, DROP[0])
    _compare(_device(a8, dev, inp, *NONE), _reference(g, inp, *NONE), torch.float32, 0.0)
    # the window-owner passes of the op without a bias still launch after a bias call asked for their decision only
    assert {"attn_bwd_row", "attn_bwd_col"} <= prof_tags(plain)
    _lib.tune("attn_rows", 0)          # forbidden: the composed form
    tags = prof_tags(lambda: _device(a8, dev, inp, *DROP))
    assert "attn_bias_add" in tags and not (FAST_BWD & tags), tags


# ---- 6. b = 0 against the op without a bias ----------------------------------------------------------------------------------
def _without_bias(a8, dev, inp, p, seed, offset):
    Q, K, V, _, dO = (x.to(dev) for x in inp)
    o, stats = ops.attention_dropout_forward(*a8[:4], Q, K, V, p, seed, offset, 0)
    dQ, dK, dV = ops.attention_dropout_backward(*a8, Q, K, V, o, stats, dO, p, seed, offset, 0)
    torch.cuda.synchronize()
    return dict(o=o, dQ=dQ, dK=dK, dV=dV, stats=stats)


def test_zero_bias_is_the_op_without_a_bias(dev):
    plain_keys = ("o", "dQ", "dK", "dV", "stats")
    g = _hub_graph(64)
    a8 = _dev8(g.csr_args(), dev)
    try:
        for rows, h, d, dtype in ((1, 1, 64, torch.float32), (1, 1, 16, torch.float32), (0, 1, 16, torch.float32),
                                  (0, 3, 8, torch.float32), (0, 2, 8, torch.float64)):
            _lib.tune("attn_rows", rows); _lib.clear_plan_cache()
            inp = _inputs(g, h, d, dtype, seed=d)
            inp = inp[:3] + (torch.zeros_like(inp[3]),) + inp[4:]
            for drop in (NONE, DROP):
                _compare(_device(a8, dev, inp, *drop), _without_bias(a8, dev, inp, *drop), dtype, drop[0],
                         "rows=%d h=%d d=%d " % (rows, h, d), factor=2, keys=plain_keys)
        # the composed path adds the zeros to s and runs the same launches otherwise: bit for bit where nothing is summed
        # by atomics
        g = _unsplit_graph(3)
        a8 = _dev8(g.csr_args(), dev)
        _lib.tune("attn_rows", 0); _lib.clear_plan_cache()
        for h, d, dtype in ((1, 16, torch.float32), (2, 8, torch.float32), (1, 8, torch.float64)):
            inp = _inputs(g, h, d, dtype, seed=d)
            inp = inp[:3] + (torch.zeros_like(inp[3]),) + inp[4:]
            for drop in (NONE, DROP):
                x, y = _device(a8, dev, inp, *drop), _without_bias(a8, dev, inp, *drop)
                for k in plain_keys:
                    assert torch.equal(x[k], y[k]), (h, d, dtype, drop, k)
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()


# ---- 7. the autograd class and the steps ----------------------------------------------------------------------------------
def _class_step(g, inp, dev, drop, step=None, b_grad=True):
    Q, K, V = (x.to(dev).clone().requires_grad_(True) for x in inp[:3])
    b = inp[3].to(dev).clone().requires_grad_(b_grad)
    out = (step or functions.fused_attention_bias_step)(g, Q, K, V, b, inp[4].to(dev), *drop)
    o = out[-1] if isinstance(out, tuple) else out
    torch.cuda.synchronize()
    return dict(o=o.detach(), dQ=Q.grad, dK=K.grad, dV=V.grad, db=b.grad)


@pytest.mark.parametrize("h,d,hg", [(1, 64, 1), (8, 32, 2), (8, 32, 1), (4, 16, 4)])
def test_fused_bias_step_matches_the_composed_step_and_the_reference(dev, h, d, hg, monkeypatch):
    """FusedAttentionBias, several heads in head groups (the group size set as test_fused_head_groups_vs_oracle sets it):
    against the composed step, against the reference, b.grad of b's shape; without a gradient for b no db is made; the
    recompute mode of the head groups gives the same numbers."""
    g = random_graph(800, 800, 14000, seed=3 + h + d, chunk_size=32, zero_rows=0.1, hub=900)   # (square: the composed step's
    inp = _inputs(g, h, d, torch.float32, seed=5)                                               # SpMM returns zeros_like(V))
    gd = g.to(dev)
    monkeypatch.setattr(functions, "_head_group", lambda h_, d_, *sizes: hg)
    for drop in (NONE, DROP):
        want = _reference(g, inp, *drop)
        fused = _class_step(gd, inp, dev, drop)
        assert fused["db"].shape == inp[3].shape
        composed = _class_step(gd, inp, dev, drop, functions.attention_bias_step)
        _compare(fused, want, torch.float32, drop[0], "fused p=%g " % drop[0])
        _compare(composed, want, torch.float32, drop[0], "composed p=%g " % drop[0])
        _compare(fused, composed, torch.float32, drop[0], "fused vs composed p=%g " % drop[0], factor=2)
    if hg < h:
        monkeypatch.setenv("GRAPHOP_FUSED_HEADS", "recompute")
        _compare(_class_step(gd, inp, dev, DROP), fused, torch.float32, DROP[0], "recompute ", factor=2)
        monkeypatch.delenv("GRAPHOP_FUSED_HEADS")
    # b without a gradient: the backward is asked for no db, and the other gradients are those of the run with it
    seen = []
    real = ops.attention_bias_backward
    monkeypatch.setattr(ops, "attention_bias_backward", lambda *a: (seen.append(a[-1]), real(*a))[1])
    nodb = _class_step(gd, inp, dev, DROP, b_grad=False)
    assert nodb["db"] is None and seen and not any(seen), seen
    _compare(nodb, fused, torch.float32, DROP[0], "b without grad ", factor=2, keys=("o", "dQ", "dK", "dV"))


def test_gradcheck_fp64(dev):
    g = random_graph(12, 10, 50, seed=4, chunk_size=3, hub=8).to(dev)
    for h, d in ((1, 3), (2, 4), (5, 2)):
        inputs = tuple(x.to(dev).requires_grad_(True) for x in _inputs(g, h, d, torch.float64, seed=h)[:4])
        for drop in ((0.0, 0, 0), (0.5, 42, 3)):
            assert torch.autograd.gradcheck(
                lambda q, k, v, b: functions.FusedAttentionBias.apply(*g.csr_args(), q, k, v, b, *drop), inputs,
                nondet_tol=1e-12)   # (split rows are summed by float atomics: the order of the adds may differ)


def test_bindings_agree(dev):
    """The ctypes binding and the compiled extension run the same entry points (torch.ops.graphop holds the ops of
    graphop._SCHEMAS only; the bias form of the fused step is not among them)."""
    ext = ops.cpp_ext
    assert ext is not None, "graphop_cpp.so not built (run __graft_entry__.build())"
    g = random_graph(500, 400, 8000, seed=6, chunk_size=32, hub=900).to(dev)
    a8 = g.csr_args()
    dr = (0.6, 2 ** 63 - 1, 2 ** 32 - 1, 5)
    for h, d in ((1, 64), (1, 16), (3, 8)):
        Q, K, V, b, dO = (x.to(dev) for x in _inputs(g, h, d, torch.float32, seed=h))
        f0 = ops.attention_bias_forward(*a8[:4], Q, K, V, b, *dr)
        f1 = ext.attention_bias_forward(*a8[:4], Q, K, V, b, p=dr[0], seed=dr[1], offset=dr[2], head0=dr[3])
        for u, v in zip(f0, f1):   # (rows split over lane groups are summed by atomics, in any order)
            torch.testing.assert_close(u, v, rtol=1e-5, atol=1e-6 / (1 - dr[0]))
        b0 = ops.attention_bias_backward(*a8, Q, K, V, b, *f0, dO, *dr)
        b1 = ext.attention_bias_backward(*a8, Q, K, V, b, *f0, dO, *dr)
        assert len(b0) == len(b1) == 4 and b1[3].shape == b.shape
        for u, v in zip(b0, b1):
            torch.testing.assert_close(u, v, rtol=1e-4, atol=1e-5 / (1 - dr[0]))
        assert ext.attention_bias_backward(*a8, Q, K, V, b, *f0, dO, *dr, need_db=False)[3].numel() == 0
    with pytest.raises(RuntimeError, match="b must be"):
        ops.attention_bias_forward(*a8[:4], Q, K, V, b[:, :2].contiguous())
    with pytest.raises(RuntimeError, match="b must be"):
        ext.attention_bias_backward(*a8, Q, K, V, b[:, 0].contiguous(), *f0, dO)
    with pytest.raises(RuntimeError, match="b must be a CUDA tensor"):
        ops.attention_bias_forward(*a8[:4], Q, K, V, b.cpu())


# ---- 8. HIP-graph replay ----------------------------------------------------------------------------------------------------
def test_fused_bias_step_replays_from_a_hip_graph(dev, force_sweep):
    """One capture of forward and backward with prepared plans, replayed twice with new values in b."""
    import gc
    g = random_graph(1500, 1500, 15000, seed=3, chunk_size=32, hub=900).to(dev)
    gen = torch.Generator(device=dev).manual_seed(4)
    Q, K, V, dO = (torch.randn(1500, 64, device=dev, generator=gen) / 8 for _ in range(4))
    bs = [torch.randn(g.n_edges, device=dev, generator=gen) for _ in range(3)]
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
