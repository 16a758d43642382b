"""Pure-torch statement of the attention weights of the fused GAT and GATv2 layers (graphop.gat_attention_weights,
graphop.gatv2_attention_weights, functions.FusedGATAttentionWeights / FusedGATv2AttentionWeights), and
the inputs the CPU and GPU tests share.  CPU, autograd-able.

For edge e = (src[e], dst[e]) in EDGE-ID order, per head k:
  GAT  : s = LeakyReLU((el[src] + er[dst]) [+ ee])                       o[i] = sum_e a_e m_e V[dst[e]]
  GATv2: s = sum_c att[k, c] LeakyReLU((xl[src] + xr[dst]) [+ xe])       o[i] = sum_e a_e m_e xr[dst[e]]
  a = row-softmax(s)
step() runs the loss <o, dO> + <a, ga> through autograd.  tests/test_gat_weights_host.py holds step() against the
layer functions of gat_edge_reference.py and gatv2_edge_reference.py at 1e-12.  Bounds (none new): a at
attention_weights_reference.TOL_A, everything else at gat_edge_reference.TOL32 / gatv2_edge_reference.tol (datt against
its scale S, fused_gatv2_reference.datt_ratio), fp64 at 1e-10."""
import functools

import torch
import torch.nn.functional as F

import dropout_reference as R
import gat_edge_reference as GE
import gatv2_edge_reference as G2
from attention_weights_reference import TOL_A
from fused_gatv2_reference import FLOOR

TOL64 = dict(rtol=1e-10, atol=1e-10)
SLOPES = GE.SLOPES
FAST_H = (1, 2, 4, 8)
FAST_HD = G2.FAST
GAT, GATV2 = "gat", "gatv2"
OPERANDS = {GAT: ("el", "er", "ee", "V"), GATV2: ("xl", "xr", "xe", "att")}


def scores(kind, src, dst, a, b, e, att=None, slope=0.2):
    """(E, h) scores: a = el / xl, b = er / xr, e = ee / xe or None"""
    z = a[src] + b[dst]
    if e is not None:
        z = z + e
    if kind == GAT:
        s = F.leaky_relu(z, slope)
        return s if s.dim() == 2 else s[:, None]
    s = (F.leaky_relu(z, slope) * att).sum(-1)
    return s if s.dim() == 2 else s[:, None]


def segment_softmax(src, n_out, s):
    """s (E, h) -> a (E, h), stats (n_out, h, 2) = (m, 1 / l) with (-1e9, 0) on rows without edges"""
    h = s.size(1)
    m = torch.full((n_out, h), FLOOR, dtype=s.dtype).scatter_reduce(0, src[:, None].expand(-1, h), s.detach(), "amax")
    ex = torch.exp(s - m[src])
    den = torch.zeros((n_out, h), dtype=s.dtype).index_add(0, src, ex)
    linv = torch.where(den > 0, 1 / den, torch.zeros_like(den))
    return ex / den[src], torch.stack([m, linv.detach()], -1)


def step(kind, src, dst, n_src, ops, dO=None, ga=None, slope=0.2, p=0.0, seed=0, offset=0, dtype=torch.float64):
    """ops = (el, er, ee | None, V) or (xl, xr, xe | None, att) -> dict(o, a, s, stats, S, d<name> per operand given) in
    `dtype`, by autograd through <o, dO> + <a, ga> (either may be None: that gradient path is then absent); a in the op's
    layout ((E) for one-head operands), ga in a's; S is the scale the error of datt is measured against."""
    names = OPERANDS[kind]
    leaf = {n: (None if t is None else t.detach().to(dtype).clone().requires_grad_(True)) for n, t in zip(names, ops)}
    first, second, edge, last = (leaf[n] for n in names)
    one = first.dim() == (1 if kind == GAT else 2)
    s = scores(kind, src, dst, first, second, edge, last if kind == GATV2 else None, slope)
    s.retain_grad()
    a, stats = segment_softmax(src, n_src, s)
    h = a.size(1)
    w = a
    if p > 0:
        w = a * R.multipliers(src.numpy(), dst.numpy(), h, p, seed, offset, dtype).reshape(-1, h)
    X = last if kind == GAT else second          # the aggregated table
    X3 = X.reshape(X.size(0), h, -1)
    o = torch.zeros((n_src, h, X3.size(-1)), dtype=dtype).index_add(0, src, w[..., None] * X3[dst])
    o = o.reshape((n_src,) + tuple(X.shape[1:]))
    loss = 0
    if dO is not None:
        loss = loss + (o * dO.to(dtype)).sum()
    if ga is not None:
        loss = loss + (a * ga.to(dtype).reshape(a.shape)).sum()
    if dO is not None or ga is not None:
        loss.backward()
    out = dict(o=o.detach(), a=(a[:, 0] if one else a).detach(), s=s.detach(), stats=stats)
    for n, t in leaf.items():
        if t is not None:
            out["d" + n] = t.grad if t.grad is not None else torch.zeros_like(t)
    if kind == GATV2 and s.grad is not None:
        z = first.detach().double()[src] + second.detach().double()[dst]
        if edge is not None:
            z = z + edge.detach().double()
        lz = F.leaky_relu(z.reshape(z.size(0), h, -1), slope)
        out["S"] = (s.grad.double()[..., None] * lz).abs().sum(0).reshape(last.shape)
    return out


def restated_weights(src, s, stats):
    """the op's formula: a = exp(min(s - m, 0)) * linv"""
    return torch.exp(torch.clamp(s - stats[..., 0][src], max=0.0)) * stats[..., 1][src]


def restated_ga(kind, src, dst, n_src, n_dst, ops, a, ga, slope):
    """The gradient through a as the classes compute it: ds' = a (ga - sum_row a ga), then GAT without ee: dz = ds' t with
    t = z > 0 ? 1 : slope; with ee: z = (el + er) + ee, dz = z > 0 ? ds' : ds' * slope, dee' = dz; del' / der' = the row /
    column sums of dz.  GATv2 without xe: dxl' = att sum_j ds' t, dxr' likewise over rows, datt' = sum ds' LeakyReLU(z).
    a, ga (E, h) -> dict of (.., h[, d]) gradients"""
    first, second, edge, last = ops
    h = a.size(1)
    rows = torch.zeros((n_src, h), dtype=a.dtype).index_add(0, src, a * ga)
    ds = a * (ga - rows[src])
    if kind == GAT:
        z = first.reshape(-1, h)[src] + second.reshape(-1, h)[dst]
        if edge is not None:
            z = z + edge.reshape(-1, h)
        dz = torch.where(z > 0, ds, ds * slope)
        out = dict(del_=torch.zeros((n_src, h), dtype=a.dtype).index_add(0, src, dz),
                   der=torch.zeros((n_dst, h), dtype=a.dtype).index_add(0, dst, dz))
        if edge is not None:
            out["dee"] = dz
        return out
    assert edge is None
    d = first.size(-1)
    xl, xr, att = first.reshape(-1, h, d), second.reshape(-1, h, d), last.reshape(h, d)
    z = xl[src] + xr[dst]
    g = torch.where(z > 0, ds[..., None], ds[..., None] * slope) * att
    return dict(dxl=torch.zeros_like(xl).index_add(0, src, g), dxr=torch.zeros_like(xr).index_add(0, dst, g),
                datt=(ds[..., None] * F.leaky_relu(z, slope)).sum(0))


def ga_inputs(n_edges, h, seed, dtype=torch.float32):
    """ga ~ randn by edge id, (E) for one head else (E, h)"""
    gen = torch.Generator().manual_seed(2000 + seed)
    return torch.randn(*((n_edges,) if h == 1 else (n_edges, h)), generator=gen, dtype=torch.float64).to(dtype)


# ---- the graphs and input sets of the GPU tier --------------------------------------------------------------------------
# name -> (kind, graph maker, edge-id permutation seed or None, h, d, input seed, input kind); the makers and the input
# generators are those of gat_edge_reference.py / gatv2_edge_reference.py
def _sets():
    sets = {}
    for h, d in ((1, 64), (2, 32), (4, 16), (8, 8), (3, 8)):          # d: a pair the fused GAT forward has fast kernels for
        sets["gat_h%d" % h] = (GAT, GE.HUB_GRAPH[32], 132, h, d, 10 + h, "unit")
    for h, d in FAST_HD + [(3, 5)]:
        sets["gatv2_%d_%d" % (h, d)] = (GATV2, G2.HUB_GRAPH[32], 132, h, d, 20 + h + d, "unit")
    sets["gat_cs3"] = (GAT, GE.HUB_GRAPH[3], 103, 4, 16, 31, "unit")
    sets["gatv2_cs3"] = (GATV2, G2.HUB_GRAPH[3], 103, 4, 16, 32, "unit")
    sets["gat_rect"] = (GAT, GE.RECT_GRAPH, None, 8, 8, 33, "unit")
    sets["gatv2_rect"] = (GATV2, G2.RECT_GRAPH, None, 2, 32, 34, "unit")
    # identity edge ids: tests/test_gat_weights.py renumbers the edges of these two (the same values in another order)
    sets["gat_ids"] = (GAT, GE.HUB_GRAPH[32], None, 4, 16, 77, "unit")
    sets["gatv2_ids"] = (GATV2, G2.HUB_GRAPH[32], None, 4, 16, 77, "unit")
    sets["gat_ties"] = (GAT, GE.TIES_GRAPH, 17, 8, 16, 5, "ties")
    sets["gat_ties_h3"] = (GAT, GE.TIES_GRAPH, 17, 3, 8, 5, "ties")
    sets["gatv2_ties"] = (GATV2, G2.TIES_GRAPH, 17, 8, 16, 5, "ties")
    sets["gatv2_ties_3_5"] = (GATV2, G2.TIES_GRAPH, 17, 3, 5, 5, "ties")
    return sets


INPUT_SETS = _sets()


def _ties(kind, src, dst, inp, seed):
    """The "ties" inputs of the two reference modules with a smaller range, so that |s| < 9 holds at every slope: the
    row-side, neighbour-side and edge operands are integers in [-2, 2] (GAT) or [-1, 1] (GATv2) and the edge operand is
    -(first[i] + second[j]) on a random 30 % of the edges: z == 0 exactly there."""
    first, second, edge = inp[:3]
    gen = torch.Generator().manual_seed(3000 + seed)
    r = 2 if kind == GAT else 1
    first, second, edge = (torch.randint(-r, r + 1, t.shape, generator=gen).to(t.dtype) for t in (first, second, edge))
    pick = torch.rand(src.numel(), generator=gen) < 0.3
    edge[pick] = -(first[src] + second[dst])[pick]
    return (first, second, edge) + tuple(inp[3:])


@functools.lru_cache(maxsize=None)
def input_set(name, dtype=torch.float32):
    """-> (kind, g, src, dst, ops = (first, second, edge, last), dO, ga, h, d) of a named set, built once; (src, dst) in
    edge-id order"""
    kind, make, perm, h, d, seed, ikind = INPUT_SETS[name]
    mod = GE if kind == GAT else G2
    g, src, dst = mod.case_graph(make, perm)
    inp = mod.inputs(src, dst, g.n_src, g.n_dst, h, d, dtype, seed, ikind)
    if ikind == "ties":
        inp = _ties(kind, src, dst, inp, seed)
    if kind == GAT:
        el, er, ee, V, dO = inp
        ops = (el, er, ee, V)
    else:
        xl, xr, xe, att, dO = inp
        ops = (xl, xr, xe, att * 0.5)          # |att|^2 of a head spreads widely at d = 8: half of it keeps |s| < 9
    return kind, g, src, dst, ops, dO, ga_inputs(g.n_edges, h, seed, dtype), h, d


def with_edge(ops, edge):
    """the operands with (edge=True) or without the edge operand"""
    return ops if edge else (ops[0], ops[1], None, ops[3])


def error_ratio(got, want, rtol, atol):
    got, want = got.detach().cpu().double(), want.double().reshape(got.shape)
    if want.numel() == 0:
        return 0.0
    return float(((got - want).abs() / (atol + rtol * want.abs())).max())
