"""GPU tier of the attention weights of the fused dot-product attention ops: graphop.attention_weights,
its graphop_cpp twin, functions.FusedAttentionWeights and the two weight steps against the float64 CPU statement of the
definition (tests/attention_weights_reference.py), against each other and against the ops that already exist.  `stats`
always comes from the matching fused forward on the device; the kernels that ran are asserted through the profile tags.

Tolerances: a at TOL_A (rtol 1e-4, atol 1e-9: essentially relative, so that small weights are checked too); everything
else at attention_edge_reference.tol (fp32 rtol 1e-4 / atol 1e-5, atol times 1 / (1 - p); twice that for two fp32 results
compared with each other; fp64 rtol 1e-10 / atol 1e-10).  Graphs and inputs: attention_edge_reference.INPUT_SETS with
(b, ga) ~ randn, on which tests/test_attention_weights_host.py::test_input_condition holds torch's own fp32 arithmetic to
half these bounds."""
import ctypes
import functools
import gc

import pytest
import torch

import attention_edge_reference as E
import attention_weights_reference as W
import gat_edge_reference as GE
from custom_op_benchmark_amd import _lib, functions, graphs, graphop as ops
from gat_reference import reorder_chunks
from test_fused_attention import prof_tags, shuffled_chunk_arrays
from util import random_graph

pytestmark = pytest.mark.gpu

MODES = W.MODES
DROP, NONE = E.DROP, E.NONE
F32, F64 = torch.float32, torch.float64
TAGS = {"attn_weights_norm", "attn_weights_xe", "attn_weights_xe_generic"}


@functools.lru_cache(maxsize=None)
def _set(name):
    return W.input_set(name)


@functools.lru_cache(maxsize=None)
def _ref_a(name, mode, dtype=F32):
    """the float64 weights of a named input set and mode, computed once and shared"""
    g, (Q, K, V, xe, _), (b, _) = _set(name)
    b, xe = W.mode_operands(mode, b, xe)
    Q, K, V, b, xe = (None if x is None else x.to(dtype) for x in (Q, K, V, b, xe))
    return W.reference_step(g.src, g.dst, g.n_src, Q, K, V, None, None, b, xe)["a"]


def _dev8(a8, dev):
    return tuple(t.to(dev) for t in a8)


def _forward(a4, Q, K, V, b, xe, drop=NONE):
    """[o, stats] of the fused forward the mode names"""
    if xe is not None:
        return ops.attention_edge_forward(*a4, Q, K, V, xe, *drop)
    if b is not None:
        return ops.attention_bias_forward(*a4, Q, K, V, b, *drop)
    return ops.attention_dropout_forward(*a4, Q, K, V, *drop)


def _weights(a8, dev, inp, bga, mode, dtype=F32, mod=ops, drop=NONE):
    """a on the device, from the statistics of the matching fused forward"""
    Q, K, V, xe, _ = (x.to(dev, dtype) for x in inp)
    b, xe = W.mode_operands(mode, bga[0].to(dev, dtype), xe)
    stats = _forward(a8[:4], Q, K, V, b, xe, drop)[1]
    a = mod.attention_weights(*a8[:4], Q, K, stats, b, xe)
    torch.cuda.synchronize()
    return a


def _check_a(g_src, n_src, a, want, tol=W.TOL_A, what=""):
    a = a.cpu()
    assert a.shape == want.shape, (what, a.shape, want.shape)
    print("%sa: %.4f of the bound" % (what, E.error_ratio(a, want, **tol)))
    torch.testing.assert_close(a.double(), want.double(), **tol, msg=lambda m: what + "a: " + m)
    a2 = a.double().reshape(a.size(0), -1)
    sums = torch.zeros(n_src, a2.size(1), dtype=F64).index_add(0, g_src, a2)
    has = torch.bincount(g_src, minlength=n_src) > 0
    assert (sums[has] - 1).abs().max() <= 1e-5, what
    assert float(a.max()) <= 1.0 and float(a.min()) >= 0.0, what


def _mode_tags(tags, mode, generic=False):
    mine = tags & TAGS
    want = {"attn_weights_norm"} if mode != "edge" else {"attn_weights_xe_generic" if generic else "attn_weights_xe"}
    assert mine == want, (mode, generic, tags)
    if mode != "edge":
        assert {t for t in tags if t.startswith("sddmm_fwd")}, tags          # the SDDMM step keeps its own tags


# ---- 1. every pair of the set, in the three modes ----------------------------------------------------------------------
@pytest.mark.parametrize("rows_sorted", [True, False])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("h,d", W.HD)
def test_every_pair_matches_the_reference(dev, h, d, mode, rows_sorted):
    """a against the float64 reference at TOL_A, row sums 1 within 1e-5, a <= 1.  With xe the fast gather kernel runs,
    with sorted rows and with shuffled chunk lists (it owns no row); plain and bias run the stream pass behind the SDDMM."""
    name = "pair_%d_%d" % (h, d)
    g, inp, bga = _set(name)
    a8 = _dev8(g.csr_args() if rows_sorted else shuffled_chunk_arrays(g, seed=11), dev)
    a = _weights(a8, dev, inp, bga, mode)
    _check_a(g.src, g.n_src, a, _ref_a(name, mode), what="h=%d d=%d %s sorted=%d " % (h, d, mode, rows_sorted))
    _mode_tags(prof_tags(lambda: _weights(a8, dev, inp, bga, mode)), mode)
    assert a.dim() == (1 if h == 1 else 2)


# ---- 2. the generic routes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", [(c, m) for c in ("fp64", "h3_d5", "h1_d16", "force_generic") for m in MODES]
                         + [("misaligned_xe", "edge")])
def test_generic_routes(dev, case, mode):
    """fp64 (at TOL64), an (h, d) outside the set, force_generic and an xe that starts 4 bytes into its buffer: edge mode
    runs the generic gather kernel; plain and bias run the same stream pass in the call's dtype behind whatever SDDMM
    the dispatch picks; in order and shuffled"""
    name = {"fp64": "generic_4_16", "h3_d5": "generic_3_5", "h1_d16": "generic_1_16", "force_generic": "generic_4_16",
            "misaligned_xe": "generic_4_16"}[case]
    g, inp, bga = _set(name)
    dtype = F64 if case == "fp64" else F32
    tol = W.TOL64 if case == "fp64" else W.TOL_A
    if case == "force_generic":
        _lib.tune("force_generic", 1)
    try:
        for a8 in (_dev8(g.csr_args(), dev), _dev8(shuffled_chunk_arrays(g, seed=2), dev)):
            def run():
                if case != "misaligned_xe":
                    return _weights(a8, dev, inp, bga, mode, dtype)
                buf = torch.empty(inp[3].numel() + 1, dtype=dtype, device=dev)
                view = buf[1:].view(inp[3].shape)
                view.copy_(inp[3])
                assert view.data_ptr() % 16 == 4 and view.is_contiguous()
                Q, K, V = (x.to(dev) for x in inp[:3])
                stats = ops.attention_edge_forward(*a8[:4], Q, K, V, view)[1]
                a = ops.attention_weights(*a8[:4], Q, K, stats, None, view)
                torch.cuda.synchronize()
                return a
            a = run()
            assert a.dtype == dtype
            _check_a(g.src, g.n_src, a, _ref_a(name, mode, dtype), tol, "%s %s " % (case, mode))
            _mode_tags(prof_tags(run), mode, generic=True)
    finally:
        _lib.tune_reset()


# ---- 3. a, b and xe are addressed by edge id -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ids", ["row_identity", "column_identity", "permuted"])
def test_operands_are_addressed_by_edge_id_not_by_slot(dev, ids, mode):
    """Row-major identity (the kernels take eid == NULL), column-major identity and a random renumbering: a[e], b[e] and
    xe[e] follow the edge ids, on both surfaces, and the same b / xe rows in another order are another result"""
    g0, inp, bga = _set("edge_ids")
    g, src, dst = {"row_identity": lambda: (g0, g0.src, g0.dst), "column_identity": lambda: GE.column_identity_edge_ids(g0),
                   "permuted": lambda: GE.permute_edge_ids(g0, 5)}[ids]()
    assert torch.equal(g.eid_r, torch.arange(g.n_edges)) == (ids == "row_identity")
    a8 = _dev8(g.csr_args(), dev)
    Q, K, V, xe, _ = inp
    b, x = W.mode_operands(mode, bga[0], xe)
    want = W.reference_step(src, dst, g.n_src, Q, K, V, None, None, b, x)["a"]
    for mod in (ops, ops.cpp_ext):
        a = _weights(a8, dev, inp, bga, mode, mod=mod)
        _check_a(src, g.n_src, a, want, what="%s %s " % (ids, mode))
    _mode_tags(prof_tags(lambda: _weights(a8, dev, inp, bga, mode)), mode)
    if mode != "plain":
        perm = torch.randperm(g.n_edges, generator=torch.Generator().manual_seed(1))
        other = _weights(a8, dev, inp[:3] + (xe[perm].contiguous(),) + inp[4:], (bga[0][perm].contiguous(), bga[1]), mode)
        assert not torch.allclose(other, a, rtol=1e-2, atol=1e-4)


# ---- 4. cross-checks against ops that already exist ----------------------------------------------------------------------
def test_cross_checks(dev):
    """At the two-results tolerance: plain mode is sparse_softmax_forward(maskedmm_csr_forward(Q, K)); xe = 0 and b = 0
    are plain mode; edge mode at 1 x 64 is bias mode with b = node_mul_edge_forward(Q, xe)"""
    two = dict(rtol=2 * W.TOL_A["rtol"], atol=2 * W.TOL_A["atol"])
    g, inp, bga = _set("cross")
    a8 = _dev8(g.csr_args(), dev)
    Q, K, V, xe, _ = (x.to(dev) for x in inp)
    plain = _weights(a8, dev, inp, bga, "plain")
    composed = ops.sparse_softmax_forward(*a8[:3], ops.maskedmm_csr_forward(*a8[:4], Q, K))
    torch.testing.assert_close(plain, composed, **two)
    zero_b = _weights(a8, dev, inp, (torch.zeros_like(bga[0]), bga[1]), "bias")
    zero_xe = _weights(a8, dev, inp[:3] + (torch.zeros_like(inp[3]),) + inp[4:], bga, "edge")
    torch.testing.assert_close(zero_b, plain, **two)
    torch.testing.assert_close(zero_xe, plain, **two)
    g, inp, bga = _set("pair_1_64")
    a8 = _dev8(g.csr_args(), dev)
    Q, K, V, xe, _ = (x.to(dev) for x in inp)
    b = ops.node_mul_edge_forward(*a8[:3], Q, xe)
    edge = _weights(a8, dev, inp, bga, "edge")
    bias = _weights(a8, dev, inp, (b, bga[1]), "bias")
    torch.testing.assert_close(edge, bias, **two)
    torch.cuda.synchronize()


# ---- 5. statistics of another forward --------------------------------------------------------------------------------------
def test_statistics_of_the_window_forward(dev):
    """Plain mode, 1 x 64, with the knobs that make small plans sweepable: attention_forward takes one of its fused
    forms, whose kernels sum the score in another order than the SDDMM that recomputes it here; a still passes TOL_A and
    the clamp keeps a <= 1"""
    for k, v in (("sweep_min_kb", 0), ("window_kb", 4), ("vrow_t", 64), ("max_windows", 512), ("sweep_min_granule", 0),
                 ("walk_window_kb", 8), ("walk_window_kb_col", 8), ("walk_min_bin", 0)):
        _lib.tune(k, v)
    _lib.clear_plan_cache()
    try:
        g = random_graph(1500, 1541, 15000, seed=7, chunk_size=32, zero_rows=0.15, hub=900)
        Q, K, V, xe, _ = E.graph_inputs(g, 1, 64, F32, seed=9)
        a8 = _dev8(g.csr_args(), dev)
        q, k, v = (x.to(dev) for x in (Q, K, V))
        tags = prof_tags(lambda: ops.attention_forward(*a8[:4], q, k, v))
        assert "attn_fwd" in tags and "softmax_fwd" not in tags, tags          # a fused forward made the statistics
        stats = ops.attention_forward(*a8[:4], q, k, v)[1]
        a = ops.attention_weights(*a8[:4], q, k, stats)
        torch.cuda.synchronize()
        want = W.reference_step(g.src, g.dst, g.n_src, Q, K, V)["a"]
        _check_a(g.src, g.n_src, a, want, what="window forward ")
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()


# ---- 6. several chunks per lane group ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_several_chunks_per_lane_group(dev, mode):
    """Chunks of one slot, enough of them that the launches give a lane group several chunks on this device, and no
    multiple of that number: the last group's run is short"""
    g, inp, bga = _set("chunky")
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    n_chunks = g.row.numel()
    cpg = min(8, max(1, n_chunks // (n_cu * 16 * 8)))          # rounds = 8, cap sddmm_cpg = 8 (xe); the norm pass caps at 16
    assert n_chunks // (n_cu * 16 * 8) >= 2 and n_chunks % cpg != 0, (n_chunks, n_cu, cpg)
    a8 = _dev8(g.csr_args(), dev)
    a = _weights(a8, dev, inp, bga, mode)
    _check_a(g.src, g.n_src, a, _ref_a("chunky", mode), what="chunky %s " % mode)
    _mode_tags(prof_tags(lambda: _weights(a8, dev, inp, bga, mode)), mode)


# ---- 7. partial chunk lists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_uncovered_edge_ids(dev, mode):
    """A row-major chunk subset (the slots of every fifth chunk move behind the last chunk, so eid / indices keep all E
    slots and no chunk covers those): through both bindings the unnamed edge ids read 0 and the rest are the covered
    sub-graph's weights; through the C ABI, which fills nothing, a pre-filled a keeps its values there"""
    g, inp, bga = _set("coverage")
    keep = [c for c in range(g.n_row_chunks) if c % 5 != 2]
    drop_c = [c for c in range(g.n_row_chunks) if c % 5 == 2]
    ptr, row, eid, idx = reorder_chunks(g.ptr_r, g.row, g.eid_r, g.indices_r, torch.tensor(keep + drop_c))
    ptr, row = ptr[:len(keep) + 1].clone(), row[:len(keep)].clone()
    covered = torch.zeros(g.n_edges, dtype=torch.bool)
    covered[eid[:int(ptr[-1])]] = True
    assert 0.1 < (~covered).double().mean() < 0.4
    a8 = _dev8((row, ptr, eid, idx, g.col, g.ptr_c, g.eid_c, g.indices_c), dev)
    plan = _lib.get_plan(*a8[:4], g.n_dst)
    assert not plan.info.full_coverage
    ids = torch.nonzero(covered)[:, 0]
    Q, K, V, xe, _ = inp
    b, x = W.mode_operands(mode, bga[0], xe)
    sub = W.reference_step(g.src[ids], g.dst[ids], g.n_src, Q, K, V, None, None,
                           None if b is None else b[ids], None if x is None else x[ids])["a"]
    want = torch.zeros(g.n_edges, 4, dtype=F64)
    want[ids] = sub
    for mod in (ops, ops.cpp_ext):
        a = _weights(a8, dev, inp, bga, mode, mod=mod).cpu()
        assert not a[~covered].any() and torch.isfinite(a).all()
        torch.testing.assert_close(a.double(), want, **W.TOL_A)
    q, k, v, xd = (t.to(dev) for t in (Q, K, V, xe))
    bd, xd = W.mode_operands(mode, bga[0].to(dev), xd)
    stats = _forward(a8[:4], q, k, v, bd, xd)[1]
    a = torch.full((g.n_edges, 4), 7.5, dtype=F32, device=dev)
    P = _lib.ptr
    _lib.check(_lib.lib().graphop_attention_weights(
        0, *(P(t) for t in a8[:4]), P(q), P(k), P(stats), P(bd) if bd is not None else None,
        P(xd) if xd is not None else None, P(a), row.numel(), g.n_edges, g.n_src, g.n_dst, 4, 16, plan.handle,
        _lib.stream_of(q)))
    torch.cuda.synchronize()
    a = a.cpu()
    assert (a[~covered] == 7.5).all()
    torch.testing.assert_close(a[covered].double(), want[covered], **W.TOL_A)


# ---- 8. the autograd class ------------------------------------------------------------------------------------------------------
def _class_step(g, inp, bga, dev, mode, drop, grads=("dO", "ga"), b_grad=True, step=None):
    Q, K, V, xe, dO = (x.to(dev) for x in inp)
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
    b, x = W.mode_operands(mode, bga[0].to(dev), xe)
    if b is not None:
        b = b.clone().requires_grad_(b_grad)
    if x is not None:
        x = x.clone().requires_grad_(True)
    ga = bga[1].to(dev) if "ga" in grads else None
    out = (step or functions.fused_attention_weights_step)(g, q, k, v, dO if "dO" in grads else None, ga, b, x, *drop)
    o, a = (out[2], out[1]) if len(out) == 3 else out
    torch.cuda.synchronize()
    zero = torch.zeros_like
    return dict(o=o.detach(), a=a.detach(), dQ=q.grad if q.grad is not None else zero(q),
                dK=k.grad if k.grad is not None else zero(k), dV=v.grad if v.grad is not None else zero(v),
                db=None if b is None else b.grad, dxe=None if x is None else x.grad, a_requires_grad=a.requires_grad)


def _compare(got, want, p, keys, what="", factor=1):
    tol = E.tol(F32, p, factor)
    for k in keys:
        x, y = got[k].cpu(), want[k].cpu()
        print("%s%s: %.3f of the bound" % (what, k, E.error_ratio(x, y, **tol)))
        torch.testing.assert_close(x.double(), y.double().reshape(x.shape), **tol, msg=lambda m: "%s%s: %s" % (what, k, m))


@pytest.mark.parametrize("p", [0.0, 0.6])
@pytest.mark.parametrize("grads", [("dO", "ga"), ("dO",), ("ga",)])
@pytest.mark.parametrize("mode,b_grad", [("plain", True), ("bias", True), ("bias", False)])
def test_class_matches_the_reference(dev, mode, b_grad, grads, p):
    """FusedAttentionWeights at 4 x 16 against autograd through the float64 reference for the loss <o, dO> + <a, ga>, with
    either gradient missing; b with and without a gradient; and, at the two-results tolerance, against the composed step"""
    g, inp, bga = _set("cross")
    gd = g.to(dev)
    drop = DROP if p > 0 else NONE
    got = _class_step(gd, inp, bga, dev, mode, drop, grads, b_grad)
    Q, K, V, xe, dO = inp
    b, _ = W.mode_operands(mode, bga[0], xe)
    want = W.reference_step(g.src, g.dst, g.n_src, Q, K, V, dO if "dO" in grads else None,
                            bga[1] if "ga" in grads else None, b, None, *drop)
    what = "%s db=%d %s p=%g " % (mode, b_grad, "+".join(grads), p)
    _check_a(g.src, g.n_src, got["a"], want["a"], what=what)
    keys = ("o", "dQ", "dK", "dV") + (("db",) if mode == "bias" and b_grad else ())
    _compare(got, want, p, keys, what)
    assert got["a_requires_grad"]
    if mode == "bias" and not b_grad:
        assert got["db"] is None
    composed = _class_step(gd, inp, bga, dev, mode, drop, grads, b_grad, functions.attention_weights_step)
    _compare(got, composed, p, keys, what + "vs composed ", factor=2)
    torch.testing.assert_close(got["a"], composed["a"], rtol=2e-4, atol=2e-9)


@pytest.mark.parametrize("mode", MODES)
def test_class_without_ga_is_the_matching_class(dev, mode):
    """o is bit for bit the matching class's o; with ga unused the backward launches exactly the matching class's
    kernels and gives its gradients; in edge mode a does not require a gradient.  The graph has no row split over
    chunks: where lane groups share a row the forward merges their pieces by float atomics in any order, and two runs
    of ONE class already differ in the last bit there (tests/test_attention_edge.py::test_need_dxe_false)."""
    g = random_graph(300, 300, 3000, seed=3, chunk_size=32)
    assert torch.bincount(g.src).max() <= 32 and torch.bincount(g.dst).max() <= 32
    inp, bga = E.graph_inputs(g, 4, 16, F32, seed=16), W.bias_inputs(g, 4, 16)
    gd = g.to(dev)
    Q, K, V, xe, dO = (x.to(dev) for x in inp)
    b, x = W.mode_operands(mode, bga[0].to(dev), xe)

    def matching(q, k, v, bb, xx):
        if mode == "edge":
            return functions.FusedAttentionEdge.apply(*gd.csr_args(), q, k, v, xx, *DROP)
        if mode == "bias":
            return functions.FusedAttentionBias.apply(*gd.csr_args(), q, k, v, bb, *DROP)
        return functions.FusedAttentionDropout.apply(*gd.csr_args(), q, k, v, *DROP)

    def leaves():
        q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
        bb = None if b is None else b.clone().requires_grad_(True)
        xx = None if x is None else x.clone().requires_grad_(True)
        return q, k, v, bb, xx

    def run(mine):
        q, k, v, bb, xx = leaves()
        if mine:
            o, a = functions.FusedAttentionWeights.apply(*gd.csr_args(), q, k, v, bb, xx, *DROP)
        else:
            o, a = matching(q, k, v, bb, xx), None
        torch.cuda.synchronize()
        tags = prof_tags(lambda: o.backward(dO))
        extra = bb if bb is not None else xx
        return o.detach(), a, tags, dict(dQ=q.grad, dK=k.grad, dV=v.grad, **({} if extra is None else {"de": extra.grad}))

    _lib.tune("attn_heads", 1); _lib.clear_plan_cache()          # the matching classes make ONE call for the four heads too
    try:
        o1, a, tags1, g1 = run(True)
        o0, _, tags0, g0 = run(False)
    finally:
        _lib.tune_reset(); _lib.clear_plan_cache()
    assert torch.equal(o1, o0)
    assert tags1 == tags0 and not (tags1 & TAGS), (tags1, tags0)
    _compare(g1, g0, DROP[0], tuple(g0), "%s vs matching class " % mode, factor=2)
    assert a.requires_grad == (mode != "edge")
    if mode == "edge":
        want = W.reference_step(g.src, g.dst, g.n_src, *inp[:3], None, None, None, inp[3])["a"]
        _check_a(g.src, g.n_src, a, want, what="class, edge mode ")


# ---- 9. HIP-graph replay ----------------------------------------------------------------------------------------------------------
def test_weights_step_replays_from_a_hip_graph(dev):
    """One capture of forward and backward (bias mode, 4 x 16, with ga) with prepared plans on a single capture stream,
    replayed twice with new values in b (the capture rules of test_edge_step_replays_from_a_hip_graph)."""
    h, d, n = 4, 16, 1500
    g = random_graph(n, n, 15000, seed=3, chunk_size=32, hub=900).to(dev)
    gen = torch.Generator(device=dev).manual_seed(4)
    Q, K, V, dO = (torch.randn(n, h, d, device=dev, generator=gen) / 4 for _ in range(4))
    bs = [torch.randn(g.n_edges, h, device=dev, generator=gen) for _ in range(3)]
    ga = torch.randn(g.n_edges, h, device=dev, generator=gen)
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
    b = bs[0].clone().requires_grad_(True)
    # nothing that earlier tests left behind (tracebacks holding device tensors and plans) may be finalised while the
    # stream is being captured: freeing a plan synchronises the device
    gc.collect()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        functions.fused_attention_weights_step(g, q, k, v, dO, ga, b, None, *DROP)
    torch.cuda.current_stream().wait_stream(side)
    q.grad = k.grad = v.grad = b.grad = None
    graph = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            o, a = functions.fused_attention_weights_step(g, q, k, v, dO, ga, b, None, *DROP)
    finally:
        gc.enable()
    p = DROP[0]
    for new in bs[1:]:
        with torch.no_grad():
            b.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        eager = _class_step(g, (Q, K, V, Q, dO), (new, ga), dev, "bias", DROP)
        torch.testing.assert_close(o.detach(), eager["o"], rtol=1e-5, atol=1e-6 / (1 - p))
        torch.testing.assert_close(a.detach(), eager["a"], rtol=1e-5, atol=1e-9)
        for key, got in (("dQ", q.grad), ("dK", k.grad), ("dV", v.grad), ("db", b.grad)):
            torch.testing.assert_close(got, eager[key], rtol=1e-4, atol=1e-5 / (1 - p))


# ---- 10. memory ----------------------------------------------------------------------------------------------------------------------
def test_weights_call_adds_only_a(dev):
    """N = 20000, E = 2 M, 4 x 16, edge mode: the attention_weights call adds at most a itself (4 E h bytes) and 4 MiB to
    the peak; the torch route would add 512 MB per (E, h, d) temporary"""
    N, E_, h, d = 20000, 2_000_000, 4, 16
    g = graphs.chung_lu_graph(N, E_, alpha=0.5, seed=3, device=dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    Q, K, V = (torch.randn(N, h, d, device=dev, generator=gen) / 4 for _ in range(3))
    xe = torch.randn(E_, h, d, device=dev, generator=gen)
    a4 = g.csr_args()[:4]
    stats = ops.attention_edge_forward(*a4, Q, K, V, xe)[1]
    for _ in range(2):
        a = ops.attention_weights(*a4, Q, K, stats, None, xe)
    del a
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    a = ops.attention_weights(*a4, Q, K, stats, None, xe)
    torch.cuda.synchronize()
    added = torch.cuda.max_memory_allocated() - base
    print("attention_weights adds %.1f MB, a is %.1f MB" % (added / 1e6, 4 * E_ * h / 1e6))
    assert added <= 4 * E_ * h + 4 * 2 ** 20, added
    assert "attn_weights_xe" in prof_tags(lambda: ops.attention_weights(*a4, Q, K, stats, None, xe))
    src = g.src.to(dev)
    sums = torch.zeros(N, h, device=dev).index_add_(0, src, a)
    has = torch.bincount(src, minlength=N) > 0
    assert float((sums[has] - 1).abs().max()) <= 1e-4 and float(a.max()) <= 1.0
