"""CPU statement of the attention weights of the fused dot-product attention ops (include/graphop_hip.h:
graphop_attention_weights), in the dtype asked for (float64 by default; the input-condition test
evaluates it in float32), built on attention_dropout_reference and attention_edge_reference; gradients come from
autograd.  For edge e = (i, j) -- i = src[e] indexes Q / o / stats, j = dst[e] indexes K / V; b, xe and a are indexed by
e -- and head k, in the three modes:

    plain: s_e = <Q_i, K_j>      bias: s_e = <Q_i, K_j> + b[e]      edge: s_e = <Q_i, K_j + xe[e]>
    a_e = softmax over the row's edges (the UNDROPPED weights)      o_i = sum_e a_e m_ek (V_j | V_j + xe[e])

`reference_step` differentiates the loss <o, dO> + <a, ga>; `restated_ga` is the ga path as FusedAttentionWeights computes
it.  `bias_inputs` draws what the GPU tier adds to attention_edge_reference's input sets."""
import torch

import attention_dropout_reference as A
import attention_edge_reference as E

TOL_A = dict(rtol=1e-4, atol=1e-9)        # for a: essentially relative, so that small weights are checked too
TOL32, TOL64 = E.TOL32, E.TOL64
MODES = ("plain", "bias", "edge")


def _two(b):
    return b if b.dim() == 2 else b[:, None]


def mode_scores(src, dst, Q, K, b=None, xe=None):
    """(E, h) scores of the mode the optional operand names"""
    assert b is None or xe is None
    if xe is not None:
        return E.edge_scores(src, dst, Q, K, xe)
    s = A.scores(src, dst, Q, K)
    return s if b is None else s + _two(b)


def _softmax(src, n_q, s):
    m, l = A.softmax_stats(src, n_q, s)
    return torch.exp(s - m[src]) / l[src], m, l


def weights(src, dst, n_q, Q, K, b=None, xe=None):
    """a (E, h), autograd-able"""
    return _softmax(src, n_q, mode_scores(src, dst, Q, K, b, xe))[0]


def edge_shape(a, Q):
    """a (E, h) in the layout the op returns: (E) for 2-D operands"""
    return a[:, 0] if Q.dim() == 2 else a


def reference_step(src, dst, n_q, Q, K, V, dO=None, ga=None, b=None, xe=None, p=0.0, seed=0, offset=0,
                   dtype=torch.float64):
    """-> dict(a, o, dQ, dK, dV, db | dxe, stats) in `dtype` from autograd through the loss <o, dO> + <a, ga> (either may
    be None); a in the op's layout, ga in a's; stats (n_q, h, 2) = (m, 1 / l) with (0, 0), in edge mode (-1e9, 0), for
    rows without edges"""
    q, k, v = (t.to(dtype).clone().requires_grad_(True) for t in (Q, K, V))
    bb = None if b is None else b.to(dtype).clone().requires_grad_(True)
    x = None if xe is None else xe.to(dtype).clone().requires_grad_(True)
    s = mode_scores(src, dst, q, k, bb, x)
    h = s.size(1)
    a, m, l = _softmax(src, n_q, s)
    w = a
    if p > 0:
        w = a * A.head_multipliers(src.numpy(), dst.numpy(), 0, h, p, seed, offset, s.dtype)
    vals = A._three(v)[dst] if x is None else A._three(v)[dst] + A._three(x)
    o = torch.zeros((n_q, h, v.size(-1)), dtype=dtype).index_add(0, src, w[..., None] * vals)
    o = o if v.dim() == 3 else o[:, 0, :]
    loss = 0
    if dO is not None:
        loss = loss + (o * dO.to(dtype)).sum()
    if ga is not None:
        loss = loss + (a * _two(ga.to(dtype))).sum()
    if dO is not None or ga is not None:
        loss.backward()
    has = l > 0
    m0 = m.detach() if x is not None else torch.where(has, m.detach(), torch.zeros_like(m))
    stats = torch.stack([m0, torch.where(has, 1 / l.detach(), torch.zeros_like(l))], -1)
    def grad(t):          # an operand the loss does not reach (V without dO) has gradient 0
        return t.grad if t.grad is not None else torch.zeros_like(t)

    out = dict(a=edge_shape(a.detach(), Q), o=o.detach(), dQ=grad(q), dK=grad(k), dV=grad(v), stats=stats)
    if bb is not None:
        out["db"] = grad(bb)
    if x is not None:
        out["dxe"] = grad(x)
    return out


def restated_ga(src, dst, n_q, n_k, Q, K, a, ga):
    """The gradient through a as FusedAttentionWeights computes it in the plain and bias modes: ds' = a (ga - sum_row a ga)
    (a = softmax(s) whatever produced the statistics), dQ' = sum_e ds'_e K_j, dK' = sum_e ds'_e Q_i, db' = ds'.
    a, ga (E, h) -> (ds', dQ', dK') with (n, h, d) operands"""
    Q, K = A._three(Q), A._three(K)
    g = torch.zeros((n_q, a.size(1)), dtype=a.dtype).index_add(0, src, a * ga)
    ds = a * (ga - g[src])
    dQ = torch.zeros_like(Q).index_add(0, src, ds[..., None] * K[dst])
    dK = torch.zeros_like(K).index_add(0, dst, ds[..., None] * Q[src])
    return ds, dQ, dK


def bias_inputs(g, h, seed, dtype=torch.float32):
    """(b, ga) ~ randn by edge id, (E) for one head (2-D operands) else (E, h)"""
    gen = torch.Generator().manual_seed(1000 + seed)
    shape = (g.n_edges,) if h == 1 else (g.n_edges, h)
    return tuple(torch.randn(*shape, generator=gen, dtype=torch.float64).to(dtype) for _ in range(2))


def mode_operands(mode, b, xe):
    """(b, xe) as the mode gives them to the op"""
    return (b if mode == "bias" else None), (xe if mode == "edge" else None)


# the graphs and input sets of the GPU tier: attention_edge_reference's, with (b, ga) drawn from the set's input seed
INPUT_SETS = E.INPUT_SETS
HD = E.HD


def input_set(name):
    """-> (graph, (Q, K, V, xe, dO), (b, ga)) of a named set"""
    g, inp = E.input_set(name)
    _, _, h, _, dtype, seed = INPUT_SETS[name]
    return g, inp, bias_inputs(g, h, seed, dtype)
