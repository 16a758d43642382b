"""The fp32 fast kernels of the four GAT op families (GATScores, GATv2Scores, FusedGATAttention and its dropout form) at
the launch geometry large graphs get, against the float64 CPU references (gat_reference.py, gatv2_reference.py,
dropout_reference.py).

Every gather pass is a chunk driver: a lane group takes `cpg` consecutive chunks and keeps the row's operands and sums
in registers while the row id is unchanged; at a row change it flushes, zeroes and reloads, and a row that lies inside
the group's chunk range is stored instead of added.  The host picks
    cpg = clamp(n_chunks / (n_cu * (256 / G) * 8), 1, cap),  cap = sddmm_cpg (score forwards) or spmm_cpg (the rest),
so cpg > 1 needs tens of thousands of chunks.  The graphs here reach that with chunk_size 1 or 2 (chunk count, not edge
count, drives cpg), and every test first ASSERTS the cpg it mirrors from the formula, the device's CU count and the
knob values: if the heuristic moves, the tests fail on that precondition instead of passing on another path.  Kernel
names come from the launch profile, so a fall-back to the generic kernels cannot pass either.

Bounds (none new): rtol = 1e-4, atol = 1e-5 against float64; datt of GATv2 |err| <= 1e-6 * S (test_gatv2_scores.py).
test_fp32_references_sit_inside_the_bounds (no GPU) shows that torch's own fp32 evaluation of the references on these
graphs stays inside them.  The references are evaluated one head at a time, so that no float64 temporary exceeds
(E, d) values.

The module's GPU tests carry the gpu mark one by one, not through `pytestmark`: the two reference checks at the end of
the module run in the tier without a GPU."""
import functools

import pytest
import torch
import torch.nn.functional as F

import dropout_reference as R
from custom_op_benchmark_amd import _lib, graphop as ops, graphs
from gat_reference import gat_layer, gat_scores, reorder_chunks
from gatv2_reference import gatv2_datt_scale, gatv2_scores
from util import random_graph

gpu = pytest.mark.gpu

SLOPE = 0.2
TOL = dict(rtol=1e-4, atol=1e-5)
DATT_FACTOR = 1e-6
P_DROP, SEED, OFFSET = 0.3, 1234567890123, 7
FAST_HD = [(1, 64), (2, 32), (2, 64), (4, 16), (4, 32), (4, 64), (8, 8), (8, 16), (8, 32)]
CAP_HD = [(1, 64), (4, 32), (8, 32)]           # one shape per row width (64, 128, 256 floats)
LONG_ROWS = (1024, 1025, 2049, 5000)           # around the long-segment bound of the stats kernel (1024 slots)
BLOCK = 256                                    # threads of a fast workgroup
DEFAULT_N_CU = 256                             # MI355X: sizes the graphs of the reference check without a GPU
MAX_ROW_BLOCKS = 8192                          # workgroups of a GATv2 row pass at most (kGatMaxRowBlocks, host_gat.h)

FUSED_FAST = {"gat_attn_stats": "k_gat_attn_stats_f32", "gat_attn_fwd": "k_gat_attn_fwd_f32",
              "gat_attn_pack": "k_gat_attn_pack_f32", "gat_attn_bwd_row": "k_gat_attn_bwd_row_f32",
              "gat_attn_bwd_col": "k_gat_attn_bwd_col_f32"}
DROP_FAST = {"gat_attn_stats": "k_gat_attn_stats_f32", "gat_attn_drop_fwd": "k_gat_attn_drop_fwd_f32",
             "gat_attn_pack": "k_gat_attn_pack_f32", "gat_attn_drop_bwd_row": "k_gat_attn_drop_bwd_row_f32",
             "gat_attn_drop_bwd_col": "k_gat_attn_drop_bwd_col_f32"}
GATV2_FAST = {"gatv2_fwd": "k_gatv2_fwd_f32", "gatv2_bwd_row": "k_gatv2_bwd_row_f32",
              "gatv2_bwd_col": "k_gatv2_bwd_col_f32"}
GAT_FAST = {"gat_fwd": "k_gat_fwd_f32", "gat_bwd_row": "k_gat_bwd_row_f32", "gat_bwd_col": "k_gat_bwd_col_f32"}


def _generic(names, *tags):
    """`names` with the kernels of `tags` (all of them if none is given) replaced by the generic ones"""
    return {t: ("k_%s_generic" % t if not tags or t in tags else k) for t, k in names.items()}


# ---- the launch geometry, mirrored from the host dispatch ---------------------------------------------------------
def _groups_wanted(n_cu, G):
    return n_cu * (BLOCK // G) * 8


def _cpg(n_chunks, n_cu, G, cap):
    """gat_cpg (host_gat.h): the one rule of every pass of the family; a cap below 1 counts as 1"""
    return max(1, min(n_chunks // _groups_wanted(n_cu, G), max(cap, 1)))


def _grid(n_chunks, cpg, G=16):
    return -(-(-(-n_chunks // cpg)) // (BLOCK // G))


def _gat_G(h):
    return 64 if h >= 8 else 32     # GatCfg<H>::G (kernels_gat.h)


def _geometry(dev):
    """(n_cu, sddmm_cpg, spmm_cpg) as the library sees them now"""
    knobs = _lib.tune_snapshot()
    return torch.cuda.get_device_properties(dev).multi_processor_count, knobs["sddmm_cpg"], knobs["spmm_cpg"]


def _assert_cpg(g, dev, G, want, forward_want=None):
    """The precondition of a cpg test: the mirrored cpg of both orientations (cap spmm_cpg) and of the score forward
    (cap sddmm_cpg) is the intended one, and the last lane group is clipped (n_chunks % cpg != 0)."""
    n_cu, sddmm, spmm = _geometry(dev)
    for name, C in (("row-major", g.n_row_chunks), ("column-major", g.n_col_chunks)):
        got = _cpg(C, n_cu, G, spmm)
        assert got == want, ("this graph no longer reaches cpg = %d in the %s pass: %d chunks on %d CUs with G = %d "
                             "and spmm_cpg = %d give cpg = %d" % (want, name, C, n_cu, G, spmm, got))
        assert C % want != 0, "%s: %d chunks are a multiple of cpg = %d, no lane group is clipped" % (name, C, want)
    if forward_want is not None:
        got = _cpg(g.n_row_chunks, n_cu, G, sddmm)
        assert got == forward_want, ("the score forward no longer runs at cpg = %d: %d chunks on %d CUs with G = %d "
                                     "and sddmm_cpg = %d give cpg = %d" % (forward_want, g.n_row_chunks, n_cu, G,
                                                                           sddmm, got))
        assert g.n_row_chunks % forward_want != 0


# ---- graphs ----------------------------------------------------------------------------------------------------------
def _from_lengths(lens, gen, chunk_size):
    n = len(lens)
    src = torch.repeat_interleave(torch.arange(n), lens)
    dst = torch.randint(0, n + 123, (int(lens.sum()),), generator=gen)     # rectangular
    return graphs.graph_from_coo(src, dst, n, n + 123, chunk_size=chunk_size)


def profile_graph(n_chunks_wanted, seed, chunk_size=1):
    """About n_chunks_wanted row-major chunks from an explicit degree profile, shuffled over the row ids: 15 % empty
    rows, 60 % of degree 1-4 (whole rows inside one lane group: the plain-store path), the rest of degree 30-100 (rows
    that span several groups: atomics at both ends), and the four LONG_ROWS.  With chunk_size = 1 every slot is a chunk
    in both orientations.  The edge count is kept off the multiples of 2, 3 and 5, so the last lane group is clipped
    at every cpg the tests use (2, 3, 5 from the GATv2 block cap, 8 and 16)."""
    gen = torch.Generator().manual_seed(seed)
    mean = 0.6 * 2.5 + 0.25 * 65.0
    n = max(200, int(round((n_chunks_wanted * chunk_size - sum(LONG_ROWS)) / mean)))
    n_empty, n_small = int(0.15 * n), int(0.60 * n)
    lens = torch.cat([torch.zeros(n_empty, dtype=torch.int64), torch.randint(1, 5, (n_small,), generator=gen),
                      torch.randint(30, 101, (n - n_empty - n_small,), generator=gen), torch.tensor(LONG_ROWS)])
    while any(int(lens.sum()) % m == 0 for m in (2, 3, 5)):
        lens[-1] += 1
    return _from_lengths(lens[torch.randperm(len(lens), generator=gen)], gen, chunk_size)


def wide_graph(n_cu):
    """Mean degree >= 64 over the non-empty rows (degrees 40-200, the four LONG_ROWS, a tenth of the rows empty) at
    chunk_size = 2: the stats pass takes its wave-per-segment form, the gather passes run at cpg > 1."""
    gen = torch.Generator().manual_seed(77)
    n = 4000 * n_cu // DEFAULT_N_CU
    lens = torch.cat([torch.zeros(n // 10, dtype=torch.int64), torch.randint(40, 201, (n - n // 10,), generator=gen),
                      torch.tensor(LONG_ROWS)])
    return _from_lengths(lens[torch.randperm(len(lens), generator=gen)], gen, 2)


@functools.lru_cache(maxsize=None)
def _graph(kind, n_cu, G=16, cpg=0):
    """One graph per (kind, lane-group width, intended cpg), built once per module run.  "cpg": the middle of the chunk
    range that gives `cpg` below the cap; "cap": past the point where spmm_cpg = 16 caps it for G = 16 (and so for the
    wider groups of GATScores); "wide": wide_graph; "small": a graph for the alignment fall-backs."""
    if kind == "cpg":
        return profile_graph(int((cpg + 0.5) * _groups_wanted(n_cu, G)), seed=100 * G + cpg)
    if kind == "cap":
        return profile_graph(int(17.5 * _groups_wanted(n_cu, 16)), seed=5)
    if kind == "wide":
        return wide_graph(n_cu)
    assert kind == "small"
    return random_graph(600, 723, 7200, seed=91, chunk_size=32, zero_rows=0.1, hub=1100)


@functools.lru_cache(maxsize=None)
def _on_device(key, dev):
    return _graph(*key).to(torch.device(dev))


def _sweep_key(dev, cpg, G=16):
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    return ("cap", n_cu) if cpg == 16 else ("cpg", n_cu, G, cpg)


def reorder_chunks_vectorised(indptr, row, eid, indices, order):
    """gat_reference.reorder_chunks for a permutation `order`, without its Python loop over the chunks"""
    lens = (indptr[1:] - indptr[:-1])[order]
    new_ptr = torch.zeros(len(order) + 1, dtype=torch.int64)
    new_ptr[1:] = torch.cumsum(lens, 0)
    slots = torch.repeat_interleave(indptr[:-1][order] - new_ptr[:-1], lens) + torch.arange(int(new_ptr[-1]))
    return new_ptr, row[order].clone(), eid[slots].clone(), indices[slots].clone()


@functools.lru_cache(maxsize=None)
def _shuffled_csr(key, dev):
    """The chunk lists of both orientations in random order, on the device: (csr_args, plan_r, plan_c)"""
    g = _graph(*key)
    gen = torch.Generator().manual_seed(1)
    pr = reorder_chunks_vectorised(g.ptr_r, g.row, g.eid_r, g.indices_r, torch.randperm(g.n_row_chunks, generator=gen))
    pc = reorder_chunks_vectorised(g.ptr_c, g.col, g.eid_c, g.indices_c, torch.randperm(g.n_col_chunks, generator=gen))
    csr = tuple(t.to(torch.device(dev)) for t in (pr[1], pr[0], pr[2], pr[3], pc[1], pc[0], pc[2], pc[3]))
    return csr, _lib.get_plan(*csr[:4], g.n_dst), _lib.get_plan(*csr[4:], g.n_src)


# ---- inputs and float64 references, one head at a time --------------------------------------------------------------
def _heads(t, node_dims):
    """[(select head k of a tensor shaped like t)] and the inverse: a tensor with no head axis is its own one head"""
    if t.dim() == node_dims:
        return [lambda x: x], lambda xs: xs[0]
    return [(lambda x, k=k: x[:, k]) for k in range(t.size(1))], lambda xs: torch.stack(xs, 1)


def _fused_inputs(g, h, d, seed):
    gen = torch.Generator().manual_seed(seed)
    shape = (lambda n: (n,) if h == 1 else (n, h))
    vs = (lambda n: (n, d) if h == 1 else (n, h, d))
    el, er = torch.randn(shape(g.n_src), generator=gen), torch.randn(shape(g.n_dst), generator=gen)
    return el, er, torch.randn(vs(g.n_dst), generator=gen), torch.randn(vs(g.n_src), generator=gen)


def _gatv2_inputs(g, h, d, seed):
    gen = torch.Generator().manual_seed(seed)
    ns = (lambda n: (n, d) if h == 1 else (n, h, d))
    xl, xr = torch.randn(ns(g.n_src), generator=gen), torch.randn(ns(g.n_dst), generator=gen)
    att = torch.randn(ns(1)[1:], generator=gen) / d ** 0.5
    return xl, xr, att, torch.randn((g.n_edges,) if h == 1 else (g.n_edges, h), generator=gen)


def _gat_inputs(g, h, seed):
    gen = torch.Generator().manual_seed(seed)
    shape = (lambda n: (n,) if h == 1 else (n, h))
    return (torch.randn(shape(g.n_src), generator=gen), torch.randn(shape(g.n_dst), generator=gen),
            torch.randn(shape(g.n_edges), generator=gen))


def masked_gat_layer_one_head(src, dst, n_out, el, er, V, negative_slope, mult):
    """dropout_reference.gat_layer_dropout for ONE head whose multipliers m[e] are given (a head's keep decisions depend
    on its index k, so a head cannot be handed to gat_layer_dropout as a one-head layer): el, er 1-D, V (n, d)."""
    s = gat_scores(src, dst, el, er, negative_slope)
    m = torch.full((n_out,), float("-inf"), dtype=s.dtype).scatter_reduce(0, src, s.detach(), "amax")
    ex = torch.exp(s - m[src])
    den = torch.zeros(n_out, dtype=s.dtype).index_add(0, src, ex)
    a = ex / den[src] * mult
    return torch.zeros((n_out, V.size(-1)), dtype=V.dtype).index_add(0, src, a[:, None] * V[dst])


def fused_reference(g, el, er, V, dO, p=0.0, dtype=torch.float64):
    """(o, del, der, dV) of the GAT layer (p = 0: gat_reference.gat_layer; else with the multipliers of
    dropout_reference.multipliers for SEED, OFFSET) by autograd in `dtype`, one head at a time"""
    sel, join = _heads(el, 1)
    mult = R.multipliers(g.src.numpy(), g.dst.numpy(), len(sel), p, SEED, OFFSET, dtype) if p > 0 else None
    outs = ([], [], [], [])
    for k, head in enumerate(sel):
        r = [head(x).to(dtype).clone().requires_grad_(True) for x in (el, er, V)]
        if mult is None:
            o = gat_layer(g.src, g.dst, g.n_src, r[0], r[1], r[2], SLOPE)
        else:
            o = masked_gat_layer_one_head(g.src, g.dst, g.n_src, r[0], r[1], r[2], SLOPE, mult[:, k])
        o.backward(head(dO).to(dtype))
        for lst, t in zip(outs, (o.detach(), r[0].grad, r[1].grad, r[2].grad)):
            lst.append(t)
    return tuple(join(ts) for ts in outs)


def gatv2_reference(g, xl, xr, att, dy, dtype=torch.float64):
    """(y, dxl, dxr, datt, S) by autograd in `dtype`, one head at a time; S, the scale datt's error is measured against,
    always in float64"""
    sel, join = _heads(xl, 2)
    outs = ([], [], [], [], [])
    for k, head in enumerate(sel):
        att_k, dy_k = (att, dy) if xl.dim() == 2 else (att[k], dy[:, k])
        r = [t.to(dtype).clone().requires_grad_(True) for t in (head(xl), head(xr), att_k)]
        y = gatv2_scores(g.src, g.dst, r[0], r[1], r[2], SLOPE)
        y.backward(dy_k.to(dtype))
        S = gatv2_datt_scale(g.src, g.dst, head(xl), head(xr), dy_k, SLOPE)
        for lst, t in zip(outs, (y.detach(), r[0].grad, r[1].grad, r[2].grad, S)):
            lst.append(t)
    stack0 = (lambda xs: xs[0]) if xl.dim() == 2 else (lambda xs: torch.stack(xs, 0))
    return join(outs[0]), join(outs[1]), join(outs[2]), stack0(outs[3]), stack0(outs[4])


def gat_reference(g, el, er, dy, dtype=torch.float64):
    """(y, del, der) of the GAT scores by autograd in `dtype`"""
    r = [t.to(dtype).clone().requires_grad_(True) for t in (el, er)]
    y = gat_scores(g.src, g.dst, r[0], r[1], SLOPE)
    y.backward(dy.to(dtype))
    return y.detach(), r[0].grad, r[1].grad


def _fused_case(key, h, d, p=0.0):
    return _fused_case_cached(key, h, d, float(p))


@functools.lru_cache(maxsize=None)
def _fused_case_cached(key, h, d, p):
    g = _graph(*key)
    inputs = _fused_inputs(g, h, d, seed=h * 100 + d)
    return inputs, fused_reference(g, *inputs, p)


@functools.lru_cache(maxsize=None)
def _gatv2_case(key, h, d):
    g = _graph(*key)
    inputs = _gatv2_inputs(g, h, d, seed=h * 100 + d + 1)
    return inputs, gatv2_reference(g, *inputs)


@functools.lru_cache(maxsize=None)
def _gat_case(key, h):
    g = _graph(*key)
    inputs = _gat_inputs(g, h, seed=h + 2)
    return inputs, gat_reference(g, *inputs)


# ---- running the ops with the launch profile on ------------------------------------------------------------------
def _profiled(fn):
    """-> (fn(), {tag: kernel name} of what it launched)"""
    _lib.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        prof = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    return out, {tag: rec["kernel"] for tag, rec in prof.items()}


def _assert_kernels(names, want, what=""):
    got = {t: names.get(t) for t in want}
    assert got == want, "%swrong kernels: %s" % (what, got)


def _run_fused(a8, dev, inputs, p=0.0):
    el, er, V, dO = (x.to(dev) for x in inputs)

    def go():
        if p > 0:
            o, stats = ops.gat_attention_dropout_forward(*a8[:4], el, er, V, SLOPE, p, SEED, OFFSET)
            return [o] + ops.gat_attention_dropout_backward(*a8, el, er, V, o, stats, dO, SLOPE, p, SEED, OFFSET)
        o, stats = ops.gat_attention_forward(*a8[:4], el, er, V, SLOPE)
        return [o] + ops.gat_attention_backward(*a8, el, er, V, o, stats, dO, SLOPE)
    return _profiled(go)


def _run_gatv2(a8, dev, inputs):
    xl, xr, att, dy = (x.to(dev) for x in inputs)
    return _profiled(lambda: [ops.gatv2_scores_forward(*a8[:4], xl, xr, att, SLOPE)]
                     + ops.gatv2_scores_backward(*a8, xl, xr, att, dy, SLOPE))


def _run_gat(a8, dev, inputs):
    el, er, dy = (x.to(dev) for x in inputs)
    return _profiled(lambda: [ops.gat_scores_forward(*a8[:4], el, er, SLOPE)]
                     + ops.gat_scores_backward(*a8, el, er, dy, SLOPE))


def _ratio(got, want):
    """max |got - want| / (atol + rtol * |want|): <= 1 is inside TOL"""
    want = want.double()
    if want.numel() == 0:
        return 0.0
    return float(((got.cpu().double() - want).abs() / (TOL["atol"] + TOL["rtol"] * want.abs())).max())


def _compare(names, got, want, what):
    for name, x, y in zip(names, got, want):
        assert x.dtype == torch.float32 and x.shape == y.shape, (what, name, x.dtype, x.shape, y.shape)
        print("%s %s: %.3f of the bound" % (what, name, _ratio(x, y)))
    for name, x, y in zip(names, got, want):
        torch.testing.assert_close(x.cpu().double(), y.double(), **TOL, msg=lambda m: "%s %s: %s" % (what, name, m))


def _datt_ratio(got, ref, S):
    return float(((got.cpu().double() - ref.double()).abs() / (DATT_FACTOR * S).clamp_min(1e-300)).max())


def _compare_gatv2(got, want, what):
    _compare(("y", "dxl", "dxr"), got[:3], want[:3], what)
    ratio = _datt_ratio(got[3], want[3], want[4])
    print("%s datt: %.3f of the bound" % (what, ratio))
    assert got[3].shape == want[3].shape and ratio <= 1.0, "%s datt: max |err| / S = %g" % (what, ratio * DATT_FACTOR)


def _sweep_params(shapes_small, shapes_cap):
    return [(c, s) for c in (2, 3) for s in shapes_small] + [(16, s) for s in shapes_cap]


# ---- a. the cpg sweep --------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cpg,hd", _sweep_params(FAST_HD, CAP_HD))
def test_fused_gat_at_cpg(dev, cpg, hd):
    """o, del, der, dV of the fused GAT layer with every gather pass at cpg in {2, 3, 16}: the row-change branch, the
    plain store of a row inside a group and the clipped last group all run."""
    key = _sweep_key(dev, cpg)
    g = _on_device(key, str(dev))
    _assert_cpg(g, dev, 16, cpg)
    for plan in (_lib.get_plan(g.row, g.ptr_r, g.eid_r, g.indices_r, g.n_dst),
                 _lib.get_plan(g.col, g.ptr_c, g.eid_c, g.indices_c, g.n_src)):
        assert plan.info.row_owned and plan.info.rows_sorted, "the plan does not own its rows: no plain stores"
    inputs, want = _fused_case(key, *hd)
    got, names = _run_fused(g.csr_args(), dev, inputs)
    _assert_kernels(names, FUSED_FAST)
    _compare(("o", "del", "der", "dV"), got, want, "cpg=%d %s" % (cpg, hd))


@gpu
@pytest.mark.parametrize("cpg,hd", _sweep_params(FAST_HD, CAP_HD))
def test_gatv2_scores_at_cpg(dev, cpg, hd):
    """y, dxl, dxr, datt of the GATv2 scores; the forward sits at its sddmm_cpg cap of 8 on the cap graph."""
    key = _sweep_key(dev, cpg)
    g = _on_device(key, str(dev))
    _assert_cpg(g, dev, 16, cpg, forward_want=min(cpg, 8))
    n_cu, _, spmm = _geometry(dev)
    assert _grid(g.n_row_chunks, _cpg(g.n_row_chunks, n_cu, 16, spmm)) <= MAX_ROW_BLOCKS     # the block cap is idle here
    inputs, want = _gatv2_case(key, *hd)
    got, names = _run_gatv2(g.csr_args(), dev, inputs)
    _assert_kernels(names, GATV2_FAST)
    _compare_gatv2(got, want, "cpg=%d %s" % (cpg, hd))


@gpu
@pytest.mark.parametrize("cpg,h", _sweep_params((1, 2, 4, 8, 16), (1, 8)))
def test_gat_scores_at_cpg(dev, cpg, h):
    """y, del, der of the GAT scores: lane groups of 32 (h <= 4) or 64 lanes, so each width has its own graphs below the
    cap.  The forward is also bit-equal to torch's fp32 leaky_relu, as at cpg = 1 (test_gat_scores.py)."""
    G = _gat_G(h)
    key = _sweep_key(dev, cpg, G)
    g = _on_device(key, str(dev))
    _assert_cpg(g, dev, G, cpg, forward_want=min(cpg, 8))
    inputs, want = _gat_case(key, h)
    got, names = _run_gat(g.csr_args(), dev, inputs)
    _assert_kernels(names, GAT_FAST)
    g0 = _graph(*key)
    assert torch.equal(got[0].cpu(), F.leaky_relu(inputs[0][g0.src] + inputs[1][g0.dst], SLOPE)), "forward not bitwise"
    _compare(("y", "del", "der"), got, want, "cpg=%d h=%d" % (cpg, h))


# ---- b. dropout ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cpg", [3, 16])
@pytest.mark.parametrize("hd", [(1, 64), (4, 16), (8, 8), (8, 32)])
def test_fused_gat_dropout_at_cpg(dev, cpg, hd):
    """The DROP = true instantiations at p = 0.3 with a fixed seed and offset.  Eight heads take two Philox blocks per
    slot: both in one lane in (8, 8)'s forward (16 slots per batch), one per lane (the SPREAD layout) in its backward
    passes and in all of (8, 32)'s; up to four heads take one block."""
    key = _sweep_key(dev, cpg)
    g = _on_device(key, str(dev))
    _assert_cpg(g, dev, 16, cpg)
    inputs, want = _fused_case(key, *hd, P_DROP)
    got, names = _run_fused(g.csr_args(), dev, inputs, P_DROP)
    _assert_kernels(names, DROP_FAST)
    assert "gat_attn_fwd" not in names
    _compare(("o", "del", "der", "dV"), got, want, "dropout cpg=%d %s" % (cpg, hd))


# ---- c. unordered chunk lists ------------------------------------------------------------------------------------------
def _shuffled(dev, G_check=(16,)):
    """The cpg = 3 graph with the chunks of both orientations in random order: no row is owned, nearly every chunk
    boundary is a row change; -> (graph key, csr_args)"""
    key = _sweep_key(dev, 3)
    csr, plan_r, plan_c = _shuffled_csr(key, str(dev))
    for plan in (plan_r, plan_c):
        assert plan.info.row_owned == 0 and plan.info.rows_sorted == 0, "the shuffled chunk list still reads as sorted"
    n_cu, _, spmm = _geometry(dev)
    g = _graph(*key)
    for G in G_check:
        for C in (g.n_row_chunks, g.n_col_chunks):
            assert _cpg(C, n_cu, G, spmm) >= 3, "the shuffled graph no longer reaches cpg >= 3 (G = %d)" % G
    return key, csr


@gpu
@pytest.mark.parametrize("hd", [(4, 16), (1, 64)])
def test_fused_gat_unordered_chunks_at_cpg(dev, hd):
    """The OWNED = false instantiations; the stats pass needs a row_owned plan and takes its generic form."""
    key, csr = _shuffled(dev)
    inputs, want = _fused_case(key, *hd)
    got, names = _run_fused(csr, dev, inputs)
    _assert_kernels(names, _generic(FUSED_FAST, "gat_attn_stats"))
    _compare(("o", "del", "der", "dV"), got, want, "unordered %s" % (hd,))
    inputs, want = _fused_case(key, *hd, P_DROP)
    got, names = _run_fused(csr, dev, inputs, P_DROP)
    _assert_kernels(names, _generic(DROP_FAST, "gat_attn_stats"))
    _compare(("o", "del", "der", "dV"), got, want, "unordered dropout %s" % (hd,))


@gpu
@pytest.mark.parametrize("hd", [(4, 16), (1, 64)])
def test_gatv2_scores_unordered_chunks_at_cpg(dev, hd):
    key, csr = _shuffled(dev)
    inputs, want = _gatv2_case(key, *hd)
    got, names = _run_gatv2(csr, dev, inputs)
    _assert_kernels(names, GATV2_FAST)
    _compare_gatv2(got, want, "unordered %s" % (hd,))


@gpu
@pytest.mark.parametrize("h", [4, 1])
def test_gat_scores_unordered_chunks_at_cpg(dev, h):
    key, csr = _shuffled(dev, G_check=(_gat_G(h),))
    inputs, want = _gat_case(key, h)
    got, names = _run_gat(csr, dev, inputs)
    _assert_kernels(names, GAT_FAST)
    _compare(("y", "del", "der"), got, want, "unordered h=%d" % h)


# ---- d. the wave-per-segment stats kernel ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("hd", [(1, 64), (2, 32), (4, 16), (8, 8)])
def test_fused_gat_wide_stats(dev, hd):
    """k_gat_attn_stats_f32<H, 64>, chosen at n_edges / n_segments >= 64: the row statistics themselves against the
    float64 row maximum and 1 / sum exp(s - m), empty rows at (-1e9, 0), then the whole layer on the same graph."""
    h, d = hd
    n_cu, _, spmm = _geometry(dev)
    key = ("wide", n_cu)
    g0, g = _graph(*key), _on_device(key, str(dev))
    plan = _lib.get_plan(g.row, g.ptr_r, g.eid_r, g.indices_r, g.n_dst)
    assert plan.info.row_owned, "the stats pass needs a row_owned plan"
    assert plan.info.n_edges // plan.info.n_segments >= 64, \
        "this graph no longer takes the wave-per-segment stats kernel: %d edges in %d segments" % (
            plan.info.n_edges, plan.info.n_segments)
    assert plan.info.max_segment_len > 1024, "no long segment"
    for C in (g.n_row_chunks, g.n_col_chunks):
        assert _cpg(C, n_cu, 16, spmm) > 1
    (el, er, V, dO), want = _fused_case(key, h, d)
    (o, stats), names = _profiled(lambda: ops.gat_attention_forward(*g.csr_args()[:4], el.to(dev), er.to(dev),
                                                                   V.to(dev), SLOPE))
    assert names["gat_attn_stats"] == "k_gat_attn_stats_f32" and names["gat_attn_fwd"] == "k_gat_attn_fwd_f32", names
    s = gat_scores(g0.src, g0.dst, el.double(), er.double(), SLOPE).reshape(g0.n_edges, h)
    idx = g0.src[:, None].expand(-1, h)
    m = torch.full((g0.n_src, h), float("-inf"), dtype=torch.float64).scatter_reduce(0, idx, s, "amax")
    den = torch.zeros((g0.n_src, h), dtype=torch.float64).index_add(0, g0.src, torch.exp(s - m[g0.src]))
    empty = torch.bincount(g0.src, minlength=g0.n_src) == 0
    assert 0 < int(empty.sum()) < g0.n_src
    stats = stats.cpu()
    assert stats.shape == (g0.n_src, h, 2)
    assert bool((stats[empty][..., 0] == -1e9).all()) and not stats[empty][..., 1].any(), "empty rows moved"
    torch.testing.assert_close(stats[~empty][..., 0].double(), m[~empty], **TOL)
    torch.testing.assert_close(stats[~empty][..., 1].double(), 1.0 / den[~empty], **TOL)
    got, names = _run_fused(g.csr_args(), dev, (el, er, V, dO))
    _assert_kernels(names, FUSED_FAST)
    _compare(("o", "del", "der", "dV"), got, want, "wide %s" % (hd,))


# ---- e. the block cap of the GATv2 row pass ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("hd", [(1, 64), (8, 16)])
def test_gatv2_row_pass_block_cap(dev, hd):
    """With spmm_cpg = 1 the cap graph would launch more than 8192 workgroups in the row pass; the dispatch raises cpg
    to ceil(C / (8192 * 16)) so that the datt partials stay inside the workspace.  datt must still meet its bound."""
    key = _sweep_key(dev, 16)
    inputs, want = _gatv2_case(key, *hd)
    try:
        _lib.tune("spmm_cpg", 1)
        _lib.clear_plan_cache()
        g = _on_device(key, str(dev))
        n_cu, _, spmm = _geometry(dev)
        C = g.n_row_chunks
        assert spmm == 1 and _cpg(C, n_cu, 16, spmm) == 1
        assert _grid(C, 1) > MAX_ROW_BLOCKS, "the block cap is no longer reached: %d chunks give %d workgroups" % (
            C, _grid(C, 1))
        cpg = -(-C // (MAX_ROW_BLOCKS * (BLOCK // 16)))
        assert cpg >= 2 and _grid(C, cpg) <= MAX_ROW_BLOCKS, (C, cpg, _grid(C, cpg))
        assert ops._gatv2_workspace_values(C, *hd) >= _grid(C, cpg) * hd[0] * hd[1]
        got, names = _run_gatv2(g.csr_args(), dev, inputs)
        _assert_kernels(names, GATV2_FAST)
        _compare_gatv2(got, want, "block cap %s" % (hd,))
    finally:
        _lib.tune_reset()
        _lib.clear_plan_cache()


# ---- f. tables that are not 16-byte aligned ----------------------------------------------------------------------------
def _shifted(t):
    """t's values in a view that starts 4 bytes into its storage"""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _small(dev):
    key = ("small", 0)
    return key, _on_device(key, str(dev))


@gpu
@pytest.mark.parametrize("h", [2, 8])
def test_gat_scores_misaligned_tables_fall_back(dev, h):
    """el, er or dy 4 bytes off (items of 8 bytes at h = 2, of 16 at h = 8): the generic kernels run, same results."""
    key, g = _small(dev)
    inputs, want = _gat_case(key, h)
    _, names = _run_gat(g.csr_args(), dev, inputs)
    _assert_kernels(names, GAT_FAST, "aligned: ")
    for i, name in enumerate(("el", "er", "dy")):
        t = [x.to(dev) for x in inputs]
        t[i] = _shifted(t[i])
        got, names = _run_gat(g.csr_args(), dev, t)
        expect = _generic(GAT_FAST) if name != "dy" else _generic(GAT_FAST, "gat_bwd_row", "gat_bwd_col")
        _assert_kernels(names, expect, "%s shifted: " % name)
        _compare(("y", "del", "der"), got, want, "%s shifted" % name)


@gpu
def test_gatv2_scores_misaligned_tables_fall_back(dev):
    """xl, xr or att 4 bytes off: the generic kernels run.  dy is read one float at a time by every kernel: any
    alignment of it is served, by whichever kernels."""
    key, g = _small(dev)
    inputs, want = _gatv2_case(key, 4, 16)
    _, names = _run_gatv2(g.csr_args(), dev, inputs)
    _assert_kernels(names, GATV2_FAST, "aligned: ")
    for i, name in enumerate(("xl", "xr", "att", "dy")):
        t = [x.to(dev) for x in inputs]
        t[i] = _shifted(t[i])
        got, names = _run_gatv2(g.csr_args(), dev, t)
        if name != "dy":
            _assert_kernels(names, _generic(GATV2_FAST), "%s shifted: " % name)
        _compare_gatv2(got, want, "%s shifted" % name)


@gpu
@pytest.mark.parametrize("p", [0.0, P_DROP])
def test_fused_gat_misaligned_tables_fall_back(dev, p):
    """el, er or V 4 bytes off in both directions: every pass generic.  o, stats or dO 4 bytes off in the backward: its
    three passes generic after a fast forward."""
    key, g = _small(dev)
    h, d = (4, 16) if p == 0 else (8, 8)
    inputs, want = _fused_case(key, h, d, p)
    fast = FUSED_FAST if p == 0 else DROP_FAST
    fwd_tags = [t for t in fast if t == "gat_attn_stats" or t.endswith("_fwd")]
    bwd_tags = [t for t in fast if t not in fwd_tags]
    a8 = g.csr_args()
    drop = (p, SEED, OFFSET) if p > 0 else ()
    fwd = ops.gat_attention_dropout_forward if p > 0 else ops.gat_attention_forward
    bwd = ops.gat_attention_dropout_backward if p > 0 else ops.gat_attention_backward
    _, names = _run_fused(a8, dev, inputs, p)
    _assert_kernels(names, fast, "aligned: ")
    for i, name in enumerate(("el", "er", "V")):
        t = [x.to(dev) for x in inputs]
        t[i] = _shifted(t[i])
        got, names = _run_fused(a8, dev, t, p)
        _assert_kernels(names, _generic(fast), "%s shifted: " % name)
        _compare(("o", "del", "der", "dV"), got, want, "%s shifted" % name)
    el, er, V, dO = (x.to(dev) for x in inputs)
    for name in ("o", "stats", "dO"):
        def go():
            o, stats = fwd(*a8[:4], el, er, V, SLOPE, *drop)
            extra = dict(o=o, stats=stats, dO=dO)
            extra[name] = _shifted(extra[name])
            return [o] + bwd(*a8, el, er, V, extra["o"], extra["stats"], extra["dO"], SLOPE, *drop)
        got, names = _profiled(go)
        _assert_kernels(names, _generic(fast, *bwd_tags), "%s shifted: " % name)
        _compare(("o", "del", "der", "dV"), got, want, "%s shifted" % name)


# ---- no GPU: the references and the bounds ----------------------------------------------------------------------------
def test_fp32_references_sit_inside_the_bounds():
    """torch's own fp32 evaluation of the references on this module's graphs (sized for the 256 CUs of an MI355X) against
    the float64 one: inside rtol = 1e-4 / atol = 1e-5, and datt inside 1e-6 * S.  The inputs do not strain the tolerances
    the kernels are held to: an fp32 kernel that sums in another order has the rest of the bound as headroom."""
    cap, wide = ("cap", DEFAULT_N_CU), ("wide", DEFAULT_N_CU)
    worst = 0.0
    for key, h, d, p in ((cap, 1, 64, 0.0), (cap, 8, 8, 0.0), (cap, 8, 8, P_DROP), (wide, 4, 16, 0.0)):
        inputs, want = _fused_case(key, h, d, p)
        got = fused_reference(_graph(*key), *inputs, p, dtype=torch.float32)
        for name, x, y in zip(("o", "del", "der", "dV"), got, want):
            r = _ratio(x, y)
            worst = max(worst, r)
            print("fused %s (%d, %d) p=%g %s: %.3f of the bound" % (key[0], h, d, p, name, r))
            assert x.dtype == torch.float32 and r <= 1.0, (key[0], h, d, p, name, r)
    inputs, want = _gatv2_case(cap, 1, 64)
    got = gatv2_reference(_graph(*cap), *inputs, dtype=torch.float32)
    for name, x, y in zip(("y", "dxl", "dxr"), got, want):
        r = _ratio(x, y)
        worst = max(worst, r)
        print("gatv2 cap (1, 64) %s: %.3f of the bound" % (name, r))
        assert r <= 1.0, (name, r)
    r = _datt_ratio(got[3], want[3], want[4])
    print("gatv2 cap (1, 64) datt: %.3f of the bound" % r)
    assert r <= 1.0, r
    inputs, want = _gat_case(cap, 8)
    for name, x, y in zip(("y", "del", "der"), gat_reference(_graph(*cap), *inputs, dtype=torch.float32), want):
        r = _ratio(x, y)
        worst = max(worst, r)
        print("gat cap h=8 %s: %.3f of the bound" % (name, r))
        assert r <= 1.0, (name, r)
    print("worst: %.3f of the bound" % worst)


def test_the_modules_graphs_and_helpers():
    """The degree profile, the cpg each graph is built for (at 256 CUs and the default knobs), and the module's own
    helpers against the shared ones: reorder_chunks_vectorised == gat_reference.reorder_chunks, the per-head references
    == gat_reference.gat_layer and dropout_reference.gat_layer_dropout evaluated with all heads at once."""
    n_cu = DEFAULT_N_CU
    for G, cpg in ((16, 2), (16, 3), (32, 2), (32, 3), (64, 2), (64, 3)):
        g = _graph("cpg", n_cu, G, cpg)
        assert g.n_row_chunks == g.n_col_chunks == g.n_edges and g.n_dst == g.n_src + 123
        assert _cpg(g.n_edges, n_cu, G, 16) == cpg and g.n_edges % cpg != 0
    g = _graph("cap", n_cu)
    assert _cpg(g.n_edges, n_cu, 16, 16) == 16 and _cpg(g.n_edges, n_cu, 16, 8) == 8 and g.n_edges % 2 == 1
    assert g.n_edges // _groups_wanted(n_cu, 16) >= 17 and g.n_row_chunks == g.n_edges
    deg = torch.bincount(g.src, minlength=g.n_src)
    assert 0.14 < float((deg == 0).float().mean()) < 0.16
    assert 0.59 < float(((deg >= 1) & (deg <= 4)).float().mean()) < 0.61
    assert sorted(deg[deg > 1000].tolist())[:3] == list(LONG_ROWS[:3]) and int((deg > 1000).sum()) == 4
    w = _graph("wide", n_cu)
    wdeg = torch.bincount(w.src, minlength=w.n_src)
    assert w.n_edges // int((wdeg > 0).sum()) >= 64 and int((wdeg == 0).sum()) > 0 and w.chunk_size == 2
    assert _cpg(w.n_row_chunks, n_cu, 16, 16) > 1 and _cpg(w.n_col_chunks, n_cu, 16, 16) > 1

    s = random_graph(260, 190, 5000, seed=11, chunk_size=8, zero_rows=0.2, hub=500)
    order = torch.randperm(s.n_row_chunks, generator=torch.Generator().manual_seed(3))
    for a, b in zip(reorder_chunks_vectorised(s.ptr_r, s.row, s.eid_r, s.indices_r, order),
                    reorder_chunks(s.ptr_r, s.row, s.eid_r, s.indices_r, order)):
        assert torch.equal(a, b)
    el, er, V, dO = (x.double() for x in _fused_inputs(s, 8, 4, seed=1))
    for p in (0.0, 0.6):
        r = [x.clone().requires_grad_(True) for x in (el, er, V)]
        o = gat_layer(s.src, s.dst, s.n_src, *r, SLOPE) if p == 0 else \
            R.gat_layer_dropout(s.src, s.dst, s.n_src, *r, SLOPE, p, SEED, OFFSET)
        o.backward(dO)
        for x, y in zip(fused_reference(s, el, er, V, dO, p), (o.detach(), r[0].grad, r[1].grad, r[2].grad)):
            torch.testing.assert_close(x, y, rtol=1e-12, atol=1e-12)
    xl, xr, att, dy = (x.double() for x in _gatv2_inputs(s, 4, 8, seed=2))
    r = [x.clone().requires_grad_(True) for x in (xl, xr, att)]
    y = gatv2_scores(s.src, s.dst, *r, SLOPE)
    y.backward(dy)
    want = (y.detach(), r[0].grad, r[1].grad, r[2].grad, gatv2_datt_scale(s.src, s.dst, xl, xr, dy, SLOPE))
    for x, z in zip(gatv2_reference(s, xl, xr, att, dy), want):
        torch.testing.assert_close(x, z, rtol=1e-12, atol=1e-12)
