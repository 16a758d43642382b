"""GPU tier of the attention weights of the fused GAT and GATv2 layers: graphop.gat_attention_weights,
graphop.gatv2_attention_weights, their graphop_cpp twins, functions.FusedGATAttentionWeights /
FusedGATv2AttentionWeights and the two weight steps against the float64 CPU statement of the definition
(tests/gat_weights_reference.py) and against the ops that already exist.  `stats` always comes from the matching fused
forward on the device; the kernels that ran are asserted through the profile tags.

Tolerances: a at TOL_A (rtol 1e-4, atol 1e-9: essentially relative, so that small weights are checked too); everything
else at gat_edge_reference.TOL32 / gatv2_edge_reference.tol (fp32 rtol 1e-4 / atol 1e-5; datt against 1e-6 S); fp64 at
1e-10.  Graphs and inputs: gat_weights_reference.INPUT_SETS, on which
tests/test_gat_weights_host.py::test_input_condition holds torch's own fp32 arithmetic to half these bounds."""
import functools
import gc

import pytest
import torch

import gat_edge_reference as GE
import gatv2_edge_reference as G2
import gat_weights_reference as W
from custom_op_benchmark_amd import _lib, functions, graphs, graphop as ops
from fused_gatv2_reference import K32, datt_ratio
from gat_reference import reorder_chunks
from test_fused_attention import prof_tags, shuffled_chunk_arrays

pytestmark = pytest.mark.gpu

GAT, GATV2 = W.GAT, W.GATV2
F32, F64 = torch.float32, torch.float64
DROP, NONE = GE.DROP, (0.0, 0, 0)
TAGS = {"gat_weights", "gat_weights_generic", "gatv2_weights", "gatv2_weights_generic"}
TAG = {GAT: "gat_weights", GATV2: "gatv2_weights"}


@functools.lru_cache(maxsize=None)
def _ref_a(name, edge, slope=0.2, dtype=F32):
    """(a, stats) of the float64 reference on a named input set (its values rounded to `dtype`), computed once"""
    kind, g, src, dst, ops_, _, _, _, _ = W.input_set(name)
    o = tuple(None if t is None else t.to(dtype) for t in W.with_edge(ops_, edge))
    r = W.step(kind, src, dst, g.n_src, o, None, None, slope)
    return r["a"], r["stats"]


def _dev(ts, dev, dtype=None):
    return tuple(None if t is None else (t.to(dev) if dtype is None or not t.is_floating_point() else t.to(dev, dtype))
                 for t in ts)


def _forward(kind, a4, o, slope=0.2, drop=NONE):
    """[o, stats] of the fused forward the operands name"""
    first, second, edge, last = o
    if kind == GAT:
        if edge is not None:
            return ops.gat_edge_attention_forward(*a4, first, second, edge, last, slope, *drop)
        return ops.gat_attention_dropout_forward(*a4, first, second, last, slope, *drop)
    return ops.gatv2_attention_dropout_forward(*a4, first, second, last, slope, *drop, xe=edge)


def _weights_of(kind, a4, o, stats, slope=0.2, mod=ops):
    first, second, edge, last = o
    if kind == GAT:
        return mod.gat_attention_weights(*a4, first, second, stats, edge, slope)
    return mod.gatv2_attention_weights(*a4, first, second, last, stats, edge, slope)


def _weights(kind, a4, o, slope=0.2, mod=ops, drop=NONE):
    """(a, stats) on the device, from the statistics of the matching fused forward"""
    stats = _forward(kind, a4, o, slope, drop)[1]
    a = _weights_of(kind, a4, o, stats, slope, mod)
    torch.cuda.synchronize()
    return a, stats


def _check_a(src, n_src, a, want, stats=None, tol=W.TOL_A, what=""):
    """a against the reference, row sums of 1 and, with the statistics the call used, the clamp: a[e] <= linv[row]
    exactly, and the largest weight of every row with slots is at least linv (1 - 1e-6)"""
    a = a.cpu()
    assert a.shape == want.shape, (what, a.shape, want.shape)
    print("%sa: %.4f of the bound" % (what, W.error_ratio(a, want, **tol)))
    torch.testing.assert_close(a.double(), want.double(), **tol, msg=lambda m: what + "a: " + m)
    a2 = a.reshape(a.size(0), -1)
    sums = torch.zeros(n_src, a2.size(1), dtype=F64).index_add(0, src, a2.double())
    has = torch.bincount(src, minlength=n_src) > 0
    assert (sums[has] - 1).abs().max() <= 1e-5, what
    if stats is not None:
        linv = stats.cpu()[..., 1]
        assert bool((a2 <= linv[src]).all()) and float(a2.min()) >= 0.0 and float(linv.max()) <= 1.0, what
        top = torch.zeros_like(linv).scatter_reduce(0, src[:, None].expand(-1, a2.size(1)), a2, "amax")
        assert bool((top[has] >= linv[has] * (1 - 1e-6)).all()), what


def _tags(tags, kind, generic=False):
    assert tags & TAGS == {TAG[kind] + ("_generic" if generic else "")}, (kind, generic, tags)


# ---- 1. shapes against the float64 reference -----------------------------------------------------------------------------
GAT_SHAPES = [("gat_h%d" % h, F32, False, False) for h in W.FAST_H] + \
    [("gat_h3", F32, True, False), ("gat_h4", F64, True, False), ("gat_h8", F32, True, True),
     ("gat_rect", F32, False, False), ("gat_rect", F64, True, False), ("gat_cs3", F32, False, False)]
GATV2_SHAPES = [("gatv2_%d_%d" % hd, F32, False, False) for hd in W.FAST_HD] + \
    [("gatv2_3_5", F32, True, False), ("gatv2_4_16", F64, True, False), ("gatv2_8_16", F32, True, True),
     ("gatv2_rect", F32, False, False), ("gatv2_rect", F64, True, False), ("gatv2_cs3", F32, False, False)]


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("name,dtype,generic,force", GAT_SHAPES + GATV2_SHAPES)
def test_shapes_match_the_reference(dev, name, dtype, generic, force, edge):
    """h in {1, 2, 4, 8} / the nine (h, d) pairs run the fast kernels; h = 3 / (3, 5), fp64 and force_generic the generic
    ones; each with and without the edge operand, through both bindings.  The hub graphs (chunks of 32 and of 3) have
    empty rows and a 1500-slot hub row, whose statistics come from the long-segment forms of the forwards; the `rect`
    sets run RECT_GRAPH, 260 rows by 190 neighbours: el / xl, stats and the row ids have one size, er / xr and the
    neighbour ids another."""
    kind, g, src, dst, o, _, _, h, d = W.input_set(name)
    if "rect" in name:
        assert g.n_src > g.n_dst and int(src.max()) >= g.n_dst and o[0].size(0) == g.n_src and o[1].size(0) == g.n_dst
    else:
        assert torch.bincount(src).max() > 1024
    a4 = _dev(g.csr_args()[:4], dev)
    od = _dev(W.with_edge(o, edge), dev, dtype)
    want, _ = _ref_a(name, edge, 0.2, dtype)
    if force:
        _lib.tune("force_generic", 1)
    try:
        for mod in (ops, ops.cpp_ext):
            a, stats = _weights(kind, a4, od, mod=mod)
            assert a.dtype == dtype and a.dim() == (1 if h == 1 else 2)
            _check_a(src, g.n_src, a, want, stats, W.TOL64 if dtype == F64 else W.TOL_A, "%s edge=%d " % (name, edge))
        _tags(prof_tags(lambda: _weights(kind, a4, od)), kind, generic)
    finally:
        _lib.tune_reset()


# ---- 2. chunk lists and edge ids -----------------------------------------------------------------------------------------
def _id_case(kind, ids):
    """the input set gat_ids / gatv2_ids (identity edge ids) with its edges renumbered: the same values, the edge
    operand's rows moved with their edges"""
    _, g0, _, _, o, _, _, h, d = W.input_set("gat_ids" if kind == GAT else "gatv2_ids")
    E = g0.n_edges
    assert torch.equal(g0.eid_r, torch.arange(E))
    if ids == "identity":
        return g0, g0.src, g0.dst, o, h, d
    if ids == "permuted":
        perm = torch.randperm(E, generator=torch.Generator().manual_seed(5))
    else:          # column-major identity: eid_c' == arange(E)
        perm = torch.empty_like(g0.eid_c)
        perm[g0.eid_c] = torch.arange(E, dtype=g0.eid_c.dtype)
    g, src, dst = GE.renumber_edge_ids(g0, perm)          # edge e of g0 is edge perm[e] of g
    assert torch.equal(g.eid_c, torch.arange(E)) == (ids == "column_identity")
    edge = torch.empty_like(o[2])
    edge[perm] = o[2]
    return g, src, dst, (o[0], o[1], edge, o[3]), h, d


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("ids", ["identity", "column_identity", "permuted"])
@pytest.mark.parametrize("kind", [GAT, GATV2])
def test_operands_are_addressed_by_edge_id_not_by_slot(dev, kind, ids, edge):
    """Row-major identity (the fast kernels take eid == NULL), column-major identity and a random renumbering: a[e] and
    ee[e] / xe[e] follow the edge ids, in order and with a shuffled chunk list (the fast kernels own no row, so they take
    it too), and the same edge rows in another order are another result"""
    g, src, dst, o, h, d = _id_case(kind, ids)
    assert torch.equal(g.eid_r, torch.arange(g.n_edges)) == (ids == "identity")
    o = W.with_edge(o, edge)
    want = W.step(kind, src, dst, g.n_src, o, None, None, 0.2)["a"]
    od = _dev(o, dev)
    for a8 in (g.csr_args(), shuffled_chunk_arrays(g, seed=11)):
        a4 = _dev(a8[:4], dev)
        a, stats = _weights(kind, a4, od)
        _check_a(src, g.n_src, a, want, stats, what="%s %s edge=%d " % (kind, ids, edge))
        _tags(prof_tags(lambda: _weights(kind, a4, od)), kind)
    if edge:
        perm = torch.randperm(g.n_edges, generator=torch.Generator().manual_seed(1))
        other, _ = _weights(kind, a4, od[:2] + (od[2][perm.to(dev)].contiguous(), od[3]))
        assert not torch.allclose(other, a, rtol=1e-2, atol=1e-4)


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("kind", [GAT, GATV2])
def test_partial_chunk_list_and_null_plan(dev, kind, edge):
    """A row-major chunk subset (the slots of every fifth chunk move behind the last chunk): through both bindings the
    edge ids no slot names read 0 and the rest are the covered sub-graph's weights; through the C ABI, which fills
    nothing, a pre-filled a keeps its values there; and with plan = NULL the generic kernel gives the same weights"""
    g, src, dst, o, h, d = _id_case(kind, "permuted")
    o = W.with_edge(o, edge)
    keep = [c for c in range(g.n_row_chunks) if c % 5 != 2]
    drop_c = [c for c in range(g.n_row_chunks) if c % 5 == 2]
    ptr, row, eid, idx = reorder_chunks(g.ptr_r, g.row, g.eid_r, g.indices_r, torch.tensor(keep + drop_c))
    ptr, row = ptr[:len(keep) + 1].clone(), row[:len(keep)].clone()
    covered = torch.zeros(g.n_edges, dtype=torch.bool)
    covered[eid[:int(ptr[-1])]] = True
    assert 0.1 < (~covered).double().mean() < 0.4
    a4 = _dev((row, ptr, eid, idx), dev)
    plan = _lib.get_plan(*a4, g.n_dst)
    assert not plan.info.full_coverage
    ids = torch.nonzero(covered)[:, 0]
    sub = tuple(t[ids] if i == 2 and t is not None else t for i, t in enumerate(o))
    want = torch.zeros(g.n_edges, h, dtype=F64)
    want[ids] = W.step(kind, src[ids], dst[ids], g.n_src, sub, None, None, 0.2)["a"]
    od = _dev(o, dev)
    for mod in (ops, ops.cpp_ext):
        a = _weights(kind, a4, od, mod=mod)[0].cpu()
        assert not a[~covered].any() and torch.isfinite(a).all()
        torch.testing.assert_close(a.double(), want, **W.TOL_A)
    _tags(prof_tags(lambda: _weights(kind, a4, od)), kind)
    stats = _forward(kind, a4, od)[1]
    P = _lib.ptr
    first, second, e_, last = od

    def raw(a, plan_handle):
        if kind == GAT:
            rc = _lib.lib().graphop_gat_attention_weights(
                0, *(P(t) for t in a4), P(first), P(second), P(e_) if edge else None, P(stats), P(a), row.numel(),
                g.n_edges, g.n_src, g.n_dst, h, 0.2, plan_handle, _lib.stream_of(first))
        else:
            rc = _lib.lib().graphop_gatv2_attention_weights(
                0, *(P(t) for t in a4), P(first), P(second), P(e_) if edge else None, P(last), P(stats), P(a), row.numel(),
                g.n_edges, g.n_src, g.n_dst, h, d, 0.2, plan_handle, _lib.stream_of(first))
        _lib.check(rc)
        torch.cuda.synchronize()

    for handle, generic in ((plan.handle, False), (None, True)):
        a = torch.full((g.n_edges, h), 7.5, dtype=F32, device=dev)
        raw(a, handle)
        _tags(prof_tags(lambda: raw(a, handle)), kind, generic)
        a = a.cpu()
        assert (a[~covered] == 7.5).all()
        torch.testing.assert_close(a[covered].double(), want[covered], **W.TOL_A)


# ---- 3. slopes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("slope", W.SLOPES)
@pytest.mark.parametrize("name,generic", [("gat_ties", False), ("gat_ties_h3", True), ("gatv2_ties", False),
                                          ("gatv2_ties_3_5", True)])
def test_slopes(dev, name, generic, slope, edge):
    """SLOPES = (0.2, 0, -0.1, 1) on integer inputs with z == 0 exactly on 30 % of the edges (with the edge operand), fast
    and generic kernels"""
    kind, g, src, dst, o, _, _, h, d = W.input_set(name)
    a4 = _dev(g.csr_args()[:4], dev)
    od = _dev(W.with_edge(o, edge), dev)
    a, stats = _weights(kind, a4, od, slope)
    _check_a(src, g.n_src, a, _ref_a(name, edge, slope)[0], stats, what="%s slope=%g edge=%d " % (name, slope, edge))
    _tags(prof_tags(lambda: _weights(kind, a4, od, slope)), kind, generic)


# ---- 4. dropout: the undropped weights, and the layer's own ---------------------------------------------------------------------
@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("name", ["gat_h4", "gat_h3", "gatv2_4_16", "gatv2_3_5"])
def test_dropout_leaves_the_weights_and_they_are_the_layers_own(dev, name, edge):
    """The statistics of a forward with p = 0.3 are those of p = 0 (bit for bit where the forward repeats bit for bit: the
    fast shapes), the op gives the same bits on the same statistics, so a is bit-equal there, and
    vector_spmm_forward(a * edge_dropout_mask(...), V or xr) is the fused o within TOL32"""
    kind, g, src, dst, o, _, _, h, d = W.input_set(name)
    a4 = _dev(g.csr_args()[:4], dev)
    od = _dev(W.with_edge(o, edge), dev)
    s0, s1 = _forward(kind, a4, od)[1], _forward(kind, a4, od, 0.2, DROP)[1]
    if name in ("gat_h4", "gatv2_4_16"):          # the fast forwards repeat bit for bit
        assert torch.equal(s0, s1)
    else:
        # The generic forwards add the chunks' sums of exp(s - m) by float atomics, in an order that changes from run to
        # run: m is exact, and two fp32 sums of the same N positive terms in different orders differ by at most
        # 2 (N - 1) 2^-24 relative (each is within (N - 1) 2^-24 of the exact sum), N = the longest row
        assert torch.equal(s0[..., 0], s1[..., 0])
        n_max = int(torch.bincount(src).max())
        torch.testing.assert_close(s1[..., 1], s0[..., 1], rtol=2 * (n_max - 1) * 2.0 ** -24, atol=0)
    # the op itself: the same statistics give the same bits, whatever p the forward that made them had
    a0 = _weights_of(kind, a4, od, s0)
    assert torch.equal(a0, _weights_of(kind, a4, od, s0.clone())) and torch.equal(_weights_of(kind, a4, od, s1),
                                                                                  _weights_of(kind, a4, od, s1.clone()))
    if torch.equal(s0, s1):
        assert torch.equal(a0, _weights_of(kind, a4, od, s1))
    for drop in (NONE, DROP):
        fused = _forward(kind, a4, od, 0.2, drop)[0]
        w = a0
        if drop[0] > 0:
            w = a0 * ops.edge_dropout_mask(*a4, h, *drop, a0.dtype).reshape(a0.shape)
        X = od[3] if kind == GAT else od[1]
        composed = ops.vector_spmm_forward(*a4, w.contiguous(), X)[:g.n_src]
        torch.cuda.synchronize()
        tol = GE.TOL32 if kind == GAT else G2.tol(F32, drop[0])
        print("%s edge=%d p=%g o: %.3f of the bound" % (name, edge, drop[0], W.error_ratio(composed, fused.cpu(), **tol)))
        torch.testing.assert_close(composed, fused, **tol)


# ---- 5. the autograd classes ---------------------------------------------------------------------------------------------------
def _class_step(kind, gd, o, dO, ga, dev, grads, drop, slope=0.2, edge_grad=True):
    leaves = [None if t is None else t.to(dev).clone().requires_grad_(True) for t in o]
    if leaves[2] is not None:
        leaves[2].requires_grad_(edge_grad)
    first, second, edge, last = leaves
    dOd = dO.to(dev) if "dO" in grads else None
    gad = ga.to(dev) if "ga" in grads else None
    if kind == GAT:
        out, a = functions.fused_gat_attention_weights_step(gd, first, second, last, dOd, gad, edge, slope, *drop)
    else:
        out, a = functions.fused_gatv2_attention_weights_step(gd, first, second, last, dOd, gad, edge, slope, *drop)
    torch.cuda.synchronize()
    got = dict(o=out.detach(), a=a.detach(), a_requires_grad=a.requires_grad)
    for n, t in zip(W.OPERANDS[kind], leaves):
        if t is not None:
            got["d" + n] = t.grad
    return got


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("grads", [("dO", "ga"), ("dO",), ("ga",)])
@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("name", ["gat_h4", "gat_h3", "gat_rect", "gatv2_4_16", "gatv2_3_5", "gatv2_rect"])
def test_classes_match_the_reference(dev, name, edge, grads, p):
    """FusedGATAttentionWeights / FusedGATv2AttentionWeights against autograd through the float64 reference for the loss
    <o, dO> + <a, ga>, with either gradient missing, fast and generic shapes and the rectangular graph (260 rows, 190
    neighbours: every gradient has its own table's row count); with xe, a does not require a gradient"""
    kind, g, src, dst, o, dO, ga, h, d = W.input_set(name)
    o = W.with_edge(o, edge)
    drop = DROP if p > 0 else NONE
    frozen = kind == GATV2 and edge          # a is non-differentiable there
    if frozen and grads == ("ga",):
        got = _class_step(kind, g.to(dev), o, dO, ga, dev, (), drop)
        assert not got["a_requires_grad"]
        return
    use_ga = "ga" in grads and not frozen
    got = _class_step(kind, g.to(dev), o, dO, ga, dev, tuple(x for x in grads if x == "dO" or use_ga), drop)
    want = W.step(kind, src, dst, g.n_src, o, dO if "dO" in grads else None, ga if use_ga else None, 0.2, *drop)
    what = "%s edge=%d %s p=%g " % (name, edge, "+".join(grads), p)
    assert got["a_requires_grad"] == (not frozen)
    _check_a(src, g.n_src, got["a"], want["a"], what=what)
    tol = GE.TOL32 if kind == GAT else G2.tol(F32, p)
    for k in ["o"] + ["d" + n for n, t in zip(W.OPERANDS[kind], o) if t is not None]:
        x = got[k]
        if x is None:          # a leaf that no given gradient reaches (V without dO)
            assert k == "dV" and "dO" not in grads, (what, k)
            continue
        if k == "datt":
            r = datt_ratio(x, want[k], want["S"]) / K32
        else:
            r = W.error_ratio(x, want[k], **tol)
        print("%s%s: %.3f of the bound" % (what, k, r))
        assert r <= 1.0, (what, k, r)


def test_edge_term_without_gradient_makes_no_dee(dev):
    kind, g, src, dst, o, dO, ga, h, d = W.input_set("gat_h4")
    got = _class_step(kind, g.to(dev), o, dO, ga, dev, ("dO", "ga"), NONE, edge_grad=False)
    assert got["dee"] is None and got["del"] is not None
    want = W.step(kind, src, dst, g.n_src, o, dO, ga, 0.2)
    for k in ("del", "der", "dV"):
        assert W.error_ratio(got[k], want[k], **GE.TOL32) <= 1.0, k


# ---- 6. HIP-graph replay ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("name", ["gat_h4", "gat_h3", "gatv2_4_16", "gatv2_3_5"])
def test_ops_replay_from_a_hip_graph(dev, name, edge):
    """One single-stream capture of the op (plans prepared by a warm-up call on a side stream), replayed twice with new
    values in the operands and their statistics: both results are bit-equal to the eager call"""
    kind, g, src, dst, o, _, _, h, d = W.input_set(name)
    a4 = _dev(g.csr_args()[:4], dev)
    od = _dev(W.with_edge(o, edge), dev)
    stats = _forward(kind, a4, od)[1]
    gc.collect()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _weights_of(kind, a4, od, stats)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            a = _weights_of(kind, a4, od, stats)
    finally:
        gc.enable()
    gen = torch.Generator(device=dev).manual_seed(8)
    for _ in range(2):
        with torch.no_grad():
            od[0].copy_(torch.randn(od[0].shape, device=dev, generator=gen))
            stats.copy_(_forward(kind, a4, od)[1])
        graph.replay()
        torch.cuda.synchronize()
        eager = _weights_of(kind, a4, od, stats)
        torch.cuda.synchronize()
        assert torch.equal(a, eager)


# ---- 7. memory ------------------------------------------------------------------------------------------------------------------------
def test_weights_call_adds_only_a(dev):
    """E = 200 k, 4 x 16, GATv2 with xe: the call adds at most a itself (4 E h bytes) and 4 MiB to the peak"""
    N, E_, h, d = 20000, 200_000, 4, 16
    g = graphs.chung_lu_graph(N, E_, alpha=0.5, seed=3, device=dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    xl, xr = (torch.randn(N, h, d, device=dev, generator=gen) for _ in range(2))
    att = torch.randn(h, d, device=dev, generator=gen) / 8
    xe = torch.randn(E_, h, d, device=dev, generator=gen)
    a4 = g.csr_args()[:4]
    stats = ops.gatv2_attention_dropout_forward(*a4, xl, xr, att, xe=xe)[1]
    for _ in range(2):
        a = ops.gatv2_attention_weights(*a4, xl, xr, att, stats, xe)
    del a
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    a = ops.gatv2_attention_weights(*a4, xl, xr, att, stats, xe)
    torch.cuda.synchronize()
    added = torch.cuda.max_memory_allocated() - base
    print("gatv2_attention_weights adds %.2f MB, a is %.2f MB" % (added / 1e6, 4 * E_ * h / 1e6))
    assert added <= 4 * E_ * h + 4 * 2 ** 20, added
    assert "gatv2_weights" in prof_tags(lambda: ops.gatv2_attention_weights(*a4, xl, xr, att, stats, xe))
    src = g.src.to(dev)
    sums = torch.zeros(N, h, device=dev).index_add_(0, src, a)
    has = torch.bincount(src, minlength=N) > 0
    assert float((sums[has] - 1).abs().max()) <= 1e-4 and bool((a <= stats[..., 1][src]).all())
