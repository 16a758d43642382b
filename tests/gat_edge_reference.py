"""Pure-torch reference of the fused GAT layer with a per-edge score term (graphop.gat_edge_attention_forward /
_backward, functions.FusedGATEdgeAttention), and the inputs its CPU and GPU tests share.  CPU, autograd-able.

gat_edge_layer restates gat_reference.gat_layer with `+ ee` and an optional multiplier after the softmax
(dropout_reference.multipliers).  It takes (src, dst) in EDGE-ID order: edge e joins row src[e] and neighbour dst[e] and
owns ee[e].  permute_edge_ids renumbers the edges of a graph, so that a slot's position and its edge id differ."""
import dataclasses

import torch
import torch.nn.functional as F

import dropout_reference as R
from util import random_graph

TOL32 = dict(rtol=1e-4, atol=1e-5)       # fp32 against float64: the bounds of tests/test_fused_gat.py
TOL64 = dict(rtol=1e-10, atol=1e-10)
NAMES = ("o", "del", "der", "dee", "dV")


def gat_edge_layer(src, dst, n_out, el, er, ee, V, negative_slope, mult=None):
    """o[i] = sum_e a_e mult_e V[dst[e]] over the edges e of row i, a = softmax over those edges of
    LeakyReLU((el[src] + er[dst]) + ee).  ee is (E) with 1-D el / er, else (E, h); V (n, d) or (n, h, d); mult (E, h)."""
    s = F.leaky_relu((el[src] + er[dst]) + ee, negative_slope)
    s2 = s if s.dim() == 2 else s[:, None]
    h = s2.size(1)
    idx = src[:, None].expand(-1, h)
    m = torch.full((n_out, h), float("-inf"), dtype=s2.dtype).scatter_reduce(0, idx, s2.detach(), "amax")
    ex = torch.exp(s2 - m[src])
    den = torch.zeros((n_out, h), dtype=s2.dtype).index_add(0, src, ex)
    a = ex / den[src]
    if mult is not None:
        a = a * mult
    V3 = V if V.dim() == 3 else V[:, None, :]
    o = torch.zeros((n_out, h, V3.size(-1)), dtype=V.dtype).index_add(0, src, a[..., None] * V3[dst])
    return o if V.dim() == 3 else o[:, 0, :]


def permute_edge_ids(g, seed):
    """-> (g', src, dst): g with its edges renumbered by a random permutation (eid_r' = perm[eid_r], eid_c' =
    perm[eid_c]; the slots stay where they are), and the edge list in the new edge-id order.  seed=None keeps the ids
    (eid_r = arange(E), the eid_identity plans)."""
    if seed is None:
        return g, g.src, g.dst
    return renumber_edge_ids(g, torch.randperm(g.n_edges, generator=torch.Generator().manual_seed(seed)))


def renumber_edge_ids(g, perm):
    """-> (g', src, dst) as permute_edge_ids, for a given permutation: edge e of g is edge perm[e] of g'"""
    src, dst = torch.empty_like(g.src), torch.empty_like(g.dst)
    src[perm], dst[perm] = g.src, g.dst
    return dataclasses.replace(g, eid_r=perm[g.eid_r], eid_c=perm[g.eid_c]), src, dst


def column_identity_edge_ids(g):
    """-> (g', src, dst): the edges numbered in column-major slot order, eid_c' == arange(E), so that the plan of the
    COLUMN-major arrays says eid_identity and the row-major ids are a non-trivial permutation (the inverse of eid_c)."""
    perm = torch.empty_like(g.eid_c)
    perm[g.eid_c] = torch.arange(g.n_edges, dtype=g.eid_c.dtype)
    out = renumber_edge_ids(g, perm)
    assert torch.equal(out[0].eid_c, torch.arange(g.n_edges)) and not torch.equal(out[0].eid_r, torch.arange(g.n_edges))
    return out


def hub_row(src):
    return int(torch.bincount(src).argmax())


def inputs(src, dst, n_src, n_dst, h, d, dtype, seed, kind="unit"):
    """(el, er, ee, V, dO) on the CPU.  kind:
    "unit"  - unit-scale randn;
    "zero"  - unit-scale randn with ee = 0 (the layer without an edge term);
    "ties"  - el, er, ee small integers and ee = -(el[i] + er[j]) on a random 30 % of the edges: z == 0 exactly there;
    "large" - unit-scale randn, then ee + 50 on every edge of three rows, - 50 on three other rows and + 60 on every
              7th edge of the hub row: |z| up to about 65, the magnitude confined to a few rows."""
    gen = torch.Generator().manual_seed(seed)
    E = src.numel()
    ns = (lambda n: (n,) if h == 1 else (n, h))
    if kind == "ties":
        el = torch.randint(-3, 4, ns(n_src), generator=gen).to(dtype)
        er = torch.randint(-3, 4, ns(n_dst), generator=gen).to(dtype)
        ee = torch.randint(-3, 4, ns(E), generator=gen).to(dtype)
        pick = torch.rand(E, generator=gen) < 0.3
        ee[pick] = -(el[src] + er[dst])[pick]
    else:
        el = torch.randn(ns(n_src), generator=gen, dtype=dtype)
        er = torch.randn(ns(n_dst), generator=gen, dtype=dtype)
        ee = torch.randn(ns(E), generator=gen, dtype=dtype)
        if kind == "large":
            hub = hub_row(src)
            rows = [int(r) for r in torch.unique(src) if int(r) != hub][:6]
            for r in rows[:3]:
                ee[src == r] += 50.0
            for r in rows[3:]:
                ee[src == r] -= 50.0
            on_hub = torch.nonzero(src == hub)[:, 0]
            ee[on_hub[::7]] += 60.0
        elif kind == "zero":
            ee.zero_()
        else:
            assert kind == "unit"
    vs = (lambda n: (n, d) if h == 1 else (n, h, d))
    V = torch.randn(vs(n_dst), generator=gen, dtype=dtype)
    dO = torch.randn(vs(n_src), generator=gen, dtype=dtype)
    return el, er, ee, V, dO


def reference(src, dst, n_src, el, er, ee, V, dO, slope, p=0.0, seed=0, offset=0, dtype=torch.float64):
    """(o, del, der, dee, dV) by autograd through gat_edge_layer evaluated in `dtype`"""
    r = [x.detach().to(dtype).clone().requires_grad_(True) for x in (el, er, ee, V)]
    h = 1 if el.dim() == 1 else el.size(1)
    mult = R.multipliers(src.numpy(), dst.numpy(), h, p, seed, offset, dtype) if p > 0 else None
    o = gat_edge_layer(src, dst, n_src, r[0], r[1], r[2], r[3], slope, mult)
    o.backward(dO.to(dtype))
    return (o.detach(),) + tuple(x.grad for x in r)


def worst_ratio(got, want, tol=TOL32):
    """max over the five outputs and their elements of |got - want| / (atol + rtol |want|)"""
    worst = 0.0
    for x, y in zip(got, want):
        x, y = x.double(), y.double()
        if x.numel():
            worst = max(worst, float(((x - y).abs() / (tol["atol"] + tol["rtol"] * y.abs())).max()))
    return worst


# ---- the graphs and input sets of the GPU tests that compare against the float64 reference -----------------------------
# (name, graph, edge-id permutation seed or None, h, d, input seed, kind, slope, (p, seed, offset))
DROP = (0.3, 2 ** 32 + 12345, 7)         # a seed above 2^32 and a non-zero offset
HUB_GRAPH = {cs: (lambda cs=cs: random_graph(300, 300, 3000, seed=cs, chunk_size=cs, zero_rows=0.2, hub=1500))
             for cs in (3, 32)}
TIES_GRAPH = lambda: random_graph(200, 200, 4000, seed=7, chunk_size=8, zero_rows=0.1, hub=300)   # noqa: E731
RECT_GRAPH = lambda: random_graph(260, 190, 5000, seed=11, chunk_size=8, zero_rows=0.2, hub=500)   # noqa: E731
BIND_GRAPH = lambda: random_graph(500, 400, 8000, seed=6, chunk_size=32, hub=900)   # noqa: E731
SLOPES = (0.2, 0.0, -0.1, 1.0)


def parity_cases():
    for cs in (3, 32):
        for h in (1, 2, 3, 4, 8):
            for d in (8, 16, 32):
                yield ("parity cs=%d" % cs, HUB_GRAPH[cs], 100 + cs, h, d, h * 100 + d, "unit", 0.2, None)


def slope_cases():
    for slope in SLOPES:
        for h, d in ((8, 16), (3, 8)):
            for kind in ("ties", "large"):
                yield ("slopes", TIES_GRAPH, 17, h, d, 5, kind, slope, None)


def dropout_cases():
    for h, d in ((4, 32), (3, 8)):
        yield ("dropout", HUB_GRAPH[32], 132, h, d, 40 + h, "unit", 0.2, DROP)


def other_cases():
    yield ("identity ids", HUB_GRAPH[32], None, 4, 16, 9, "unit", 0.2, None)
    yield ("zero edge term", HUB_GRAPH[32], 132, 4, 16, 11, "zero", 0.2, None)
    for h, d in ((3, 8), (4, 16)):
        yield ("hard layouts", RECT_GRAPH, 21, h, d, h, "unit", 0.2, None)
    yield ("no dee", BIND_GRAPH, 23, 4, 16, 3, "unit", 0.2, None)


def all_cases():
    for gen in (parity_cases, slope_cases, dropout_cases, other_cases):
        yield from gen()


_GRAPHS = {}


def case_graph(make, perm_seed):
    """(g', src, dst) of a case, built once"""
    key = (make, perm_seed)
    if key not in _GRAPHS:
        _GRAPHS[key] = permute_edge_ids(make(), perm_seed)
    return _GRAPHS[key]


def case_inputs(case, dtype=torch.float64):
    _, make, perm_seed, h, d, seed, kind, _, _ = case
    g, src, dst = case_graph(make, perm_seed)
    return inputs(src, dst, g.n_src, g.n_dst, h, d, dtype, seed, kind)


def case_reference(case, inp, dtype=torch.float64):
    _, make, perm_seed, _, _, _, _, slope, drop = case
    g, src, dst = case_graph(make, perm_seed)
    p, seed, offset = drop or (0.0, 0, 0)
    return reference(src, dst, g.n_src, *inp, slope, p, seed, offset, dtype)
