"""CPU statement of the fused dot-product attention step with edge features (include/graphop_hip.h), in
the dtype asked for (float64 by default; the input-condition test evaluates it in float32), built on
attention_dropout_reference (softmax_stats, head_multipliers); gradients come from autograd.  For edge e = (i, j) --
i = src[e] indexes Q / o, j = dst[e] indexes K / V, xe is indexed by e -- and global head k:

    kx_e = K_j + xe[e]    vx_e = V_j + xe[e]    s_e = <Q_i, kx_e>    a_e = softmax over the row's edges
    o_i = sum_e a_e m_ek vx_e

The row statistics are those of the undropped scores, (-1e9, 0) for rows without edges.  `restated` is the backward as
the kernels compute it, dxe = ds Q_i + a m dO_i included.  `inputs` builds what the GPU tier feeds the op."""
import torch

import attention_dropout_reference as A

TOL32 = dict(rtol=1e-4, atol=1e-5)        # TOL[torch.float32] of tests/test_fused_attention.py
TOL64 = dict(rtol=1e-10, atol=1e-10)      # what tests/test_gatv2_edge.py uses for fp64 (fused_gatv2_reference.TOL64)
KEYS = ("o", "dQ", "dK", "dV", "dxe")


def inputs(n_q, n_k, n_edges, h, d, dtype, seed):
    """(Q, K, V, xe, dO) on the CPU: Q, dO ~ randn / sqrt(d), K, V, xe ~ randn.  A score is a sum of d products of
    variance 2 / d: |s| stays below ten or so, far from where one ulp of an fp32 score shows in exp(s - m) at rtol 1e-4
    (tests/test_attention_heads.py::test_heads_do_not_leak_into_each_other has the arithmetic).  h == 1 gives 2-D
    operands."""
    gen = torch.Generator().manual_seed(seed)
    shape = (lambda n: (n, d) if h == 1 else (n, h, d))
    Q, dO = (torch.randn(*shape(n_q), generator=gen, dtype=torch.float64).to(dtype) / d ** 0.5 for _ in range(2))
    K, V = (torch.randn(*shape(n_k), generator=gen, dtype=torch.float64).to(dtype) for _ in range(2))
    xe = torch.randn(*shape(n_edges), generator=gen, dtype=torch.float64).to(dtype)
    return Q, K, V, xe, dO


def graph_inputs(g, h, d, dtype, seed):
    return inputs(g.n_src, g.n_dst, g.n_edges, h, d, dtype, seed)


def edge_scores(src, dst, Q, K, xe):
    """(E, h) scores"""
    return (A._three(Q)[src] * (A._three(K)[dst] + A._three(xe))).sum(-1)


def attention_edge(src, dst, n_q, Q, K, V, xe, p=0.0, seed=0, offset=0, head0=0):
    """o (n_q[, h], d), autograd-able.  p = 0: no dropout."""
    s = edge_scores(src, dst, Q, K, xe)
    h = s.size(1)
    m, l = A.softmax_stats(src, n_q, s)
    a = torch.exp(s - m[src]) / l[src]
    if p > 0:
        a = a * A.head_multipliers(src.numpy(), dst.numpy(), head0, h, p, seed, offset, s.dtype)
    vx = A._three(V)[dst] + A._three(xe)
    o = torch.zeros((n_q, h, V.size(-1)), dtype=V.dtype).index_add(0, src, a[..., None] * vx)
    return o if V.dim() == 3 else o[:, 0, :]


def reference_step(src, dst, n_q, Q, K, V, xe, dO, p=0.0, seed=0, offset=0, head0=0, dtype=torch.float64):
    """-> dict(o, dQ, dK, dV, dxe, stats) in `dtype` from autograd; dxe in xe's shape; stats (n_q, h, 2) = (m, 1 / l),
    (-1e9, 0) for rows without edges"""
    q, k, v, x = (t.to(dtype).clone().requires_grad_(True) for t in (Q, K, V, xe))
    o = attention_edge(src, dst, n_q, q, k, v, x, p, seed, offset, head0)
    o.backward(dO.to(dtype))
    m, l = A.softmax_stats(src, n_q, edge_scores(src, dst, q.detach(), k.detach(), x.detach()))
    stats = torch.stack([m, torch.where(l > 0, 1 / l, torch.zeros_like(l))], -1)
    return dict(o=o.detach(), dQ=q.grad, dK=k.grad, dV=v.grad, dxe=x.grad, stats=stats)


def restated(src, dst, n_q, n_k, Q, K, V, xe, dO, mult):
    """The step as the kernels compute it, mult = m (E, h): kx and vx formed once, a from the statistics of the undropped
    scores, o of the dropped weights, D_i = <dO_i, o_i>, da = m <dO_i, vx>, ds = a (da - D_i), then the four sums.
    -> (o, D, dQ, dK, dV, dxe) with (n, h, d) operands"""
    Q, K, V, xe, dO = (A._three(x) for x in (Q, K, V, xe, dO))
    kx, vx = K[dst] + xe, V[dst] + xe
    s = (Q[src] * kx).sum(-1)
    m, l = A.softmax_stats(src, n_q, s)
    linv = torch.where(l > 0, 1 / l, torch.zeros_like(l))
    a = torch.exp(s - m[src]) * linv[src]
    am = a * mult
    o = torch.zeros_like(Q).index_add(0, src, am[..., None] * vx)
    D = (dO * o).sum(-1)
    da = mult * (dO[src] * vx).sum(-1)
    ds = a * (da - D[src])
    dQ = torch.zeros_like(Q).index_add(0, src, ds[..., None] * kx)
    dK = torch.zeros_like(K).index_add(0, dst, ds[..., None] * Q[src])
    dV = torch.zeros_like(V).index_add(0, dst, am[..., None] * dO[src])
    dxe = ds[..., None] * Q[src] + am[..., None] * dO[src]
    return o, D, dQ, dK, dV, dxe


def tol(dtype, p=0.0, factor=1):
    """the GPU tier's bound: TOL32 with atol / (1 - p) -- every term of every sum is scaled by the multiplier -- or TOL64;
    factor 2 for two fp32 results compared with each other"""
    if dtype == torch.float64:
        return dict(TOL64)
    return dict(rtol=factor * TOL32["rtol"], atol=factor * TOL32["atol"] / (1 - p))


def error_ratio(got, want, rtol, atol):
    """max over the elements of |got - want| / (atol + rtol |want|): <= 1 passes assert_close with these bounds"""
    got, want = got.double(), want.double().reshape(got.shape)
    return float(((got - want).abs() / (atol + rtol * want.abs())).max()) if got.numel() else 0.0


# ---- the graphs and input sets of the GPU tier (tests/test_attention_edge.py), named so that the CPU tier checks them ----
HD = [(1, 64), (2, 32), (2, 64), (4, 16), (4, 32), (4, 64), (8, 8), (8, 16), (8, 32)]   # GO_DISPATCH_GAT_HD
DROP = (0.6, 1234567890123, 7)
NONE = (0.0, 0, 0)


def tier_graph(seed=3):
    """rectangular, rows without edges, a hub row cut into many chunks and so split over lane groups, parallel edges"""
    from util import random_graph
    g = random_graph(300, 337, 2700, seed=seed, chunk_size=8, zero_rows=0.2, hub=150)
    deg = torch.bincount(g.src, minlength=g.n_src)
    assert g.n_src != g.n_dst and (deg == 0).any() and deg.max() >= 150 and (deg % 8 != 0).any()
    assert torch.unique(torch.stack([g.src, g.dst], 1), dim=0).size(0) < g.n_edges          # parallel edges
    return g


def chunky_graph():
    """chunks of one slot: the graph of the several-chunks-per-lane-group test"""
    from util import random_graph
    return random_graph(3000, 3000, 110000, seed=17, chunk_size=1)


# name -> (graph builder, graph seed or None, h, d, dtype, input seed)
INPUT_SETS = {"pair_%d_%d" % hd: (tier_graph, 3, hd[0], hd[1], torch.float32, hd[0] * 100 + hd[1]) for hd in HD}
INPUT_SETS.update({
    "edge_ids": (tier_graph, 9, 4, 16, torch.float32, 6),
    "cross": (tier_graph, 3, 4, 16, torch.float32, 21),
    "coverage": (tier_graph, 3, 4, 16, torch.float32, 8),
    "generic_3_5": (tier_graph, 3, 3, 5, torch.float32, 305),
    "generic_1_16": (tier_graph, 3, 1, 16, torch.float32, 116),
    "generic_4_16": (tier_graph, 3, 4, 16, torch.float32, 41),
    "leak": (tier_graph, 3, 4, 16, torch.float32, 23),
    "chunky": (chunky_graph, None, 4, 16, torch.float32, 2),
    "head0": (tier_graph, 3, 4, 16, torch.float32, 31),
    "autograd_8_32": (tier_graph, 3, 8, 32, torch.float32, 5),
})


def input_set(name):
    """-> (graph, (Q, K, V, xe, dO)) of a named set"""
    build, gseed, h, d, dtype, seed = INPUT_SETS[name]
    g = build() if gseed is None else build(gseed)
    return g, graph_inputs(g, h, d, dtype, seed)
