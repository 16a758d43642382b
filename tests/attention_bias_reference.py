"""CPU statement of the fused dot-product attention step with a per-edge score bias (include/graphop_hip.h, DESIGN.md
4.5k), in the tensors' dtype (the tests pass float64), built on attention_dropout_reference (scores, softmax_stats,
head_multipliers); gradients come from autograd.  For edge e = (i, j) -- i = src[e] indexes Q / o, j = dst[e] indexes
K / V, b is indexed by e -- and global head k:

    s_e = <Q_i, K_j> + b[e, k]     a_e = softmax over the row's edges     o_i = sum_e a_e m_ek V_j

The row statistics are those of the biased, undropped scores.  `restated` is the backward as the kernels compute it,
db = ds included."""
import torch

import attention_dropout_reference as A


def _two(b):
    return b if b.dim() == 2 else b[:, None]


def biased_scores(src, dst, Q, K, b):
    """(E, h) scores; b (E) / (E, h)"""
    return A.scores(src, dst, Q, K) + _two(b)


def attention_bias(src, dst, n_q, Q, K, V, b, p=0.0, seed=0, offset=0, head0=0):
    """o (n_q[, h], d), autograd-able.  p = 0: no dropout."""
    s = biased_scores(src, dst, Q, K, b)
    h = s.size(1)
    m, l = A.softmax_stats(src, n_q, s)
    a = torch.exp(s - m[src]) / l[src]
    if p > 0:
        a = a * A.head_multipliers(src.numpy(), dst.numpy(), head0, h, p, seed, offset, s.dtype)
    o = torch.zeros((n_q, h, V.size(-1)), dtype=V.dtype).index_add(0, src, a[..., None] * A._three(V)[dst])
    return o if V.dim() == 3 else o[:, 0, :]


def reference_step(src, dst, n_q, Q, K, V, b, dO, p=0.0, seed=0, offset=0, head0=0):
    """-> dict(o, dQ, dK, dV, db, stats) in float64 from autograd; db in b's shape; stats (n_q, h, 2) = (m, 1 / l), (0, 0)
    for empty rows"""
    q, k, v, bb = (x.double().clone().requires_grad_(True) for x in (Q, K, V, b))
    o = attention_bias(src, dst, n_q, q, k, v, bb, p, seed, offset, head0)
    o.backward(dO.double())
    m, l = A.softmax_stats(src, n_q, biased_scores(src, dst, q.detach(), k.detach(), bb.detach()))
    has = l > 0
    stats = torch.stack([torch.where(has, m, torch.zeros_like(m)), torch.where(has, 1 / l, torch.zeros_like(l))], -1)
    return dict(o=o.detach(), dQ=q.grad, dK=k.grad, dV=v.grad, db=bb.grad, stats=stats)


def restated(src, dst, n_q, n_k, Q, K, V, b, dO, mult):
    """The step as the kernels compute it, mult = m (E, h): a from the statistics of the biased, undropped scores, o of
    the dropped weights, D_i = <dO_i, o_i>, da = m <dO_i, V_j>, ds = a (da - D_i), db = ds, then the three sums.
    -> (o, D, dQ, dK, dV, db) with (n, h, d) operands and db (E, h)"""
    Q, K, V, dO = (A._three(x) for x in (Q, K, V, dO))
    s = (Q[src] * K[dst]).sum(-1) + _two(b)
    m, l = A.softmax_stats(src, n_q, s)
    linv = torch.where(l > 0, 1 / l, torch.zeros_like(l))
    a = torch.exp(s - m[src]) * linv[src]
    am = a * mult
    o = torch.zeros_like(Q).index_add(0, src, am[..., None] * V[dst])
    D = (dO * o).sum(-1)
    da = mult * (dO[src] * V[dst]).sum(-1)
    ds = a * (da - D[src])
    dQ = torch.zeros_like(Q).index_add(0, src, ds[..., None] * K[dst])
    dK = torch.zeros_like(K).index_add(0, dst, ds[..., None] * Q[src])
    dV = torch.zeros_like(V).index_add(0, dst, am[..., None] * dO[src])
    return o, D, dQ, dK, dV, ds
