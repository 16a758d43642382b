"""CPU statement of the fused dot-product attention step with dropout on the attention weights (include/graphop_hip.h,
DESIGN.md 4.5j), in the tensors' dtype (the tests pass float64), built from dropout_reference.multipliers; gradients
come from autograd.  For edge (i, j) -- i = src indexes Q / o, j = dst indexes K / V -- and global head k:

    s_ij = <Q_i, K_j>     a_ij = softmax over the row's edges     o_i = sum_j a_ij m_ijk V_j

The row statistics are those of the undropped scores.  `restated` is the backward as the kernels compute it."""
import torch

import dropout_reference as R


def head_multipliers(src, dst, g0, hg, p, seed, offset=0, dtype=torch.float64):
    """m[e, k] for the global heads g0 .. g0 + hg - 1, stated through dropout_reference.keep over all g0 + hg heads: what
    a call that handles one group of heads (head0 = g0) must apply."""
    scale = torch.tensor(1.0 / (1.0 - float(p)), dtype=torch.float64).to(dtype)
    # heads below 4 * (g0 // 4) fill whole Philox blocks of their own: leaving those blocks out shifts the block index
    # (the counter's third word) and nothing else, so a call with a large g0 need not state a million heads
    skip = g0 // 4 if g0 + hg > 64 else 0
    lo = g0 - 4 * skip
    k = torch.from_numpy(_keep_from_block(src, dst, skip, lo + hg, p, seed, offset)[:, lo:lo + hg])
    return torch.where(k, scale, torch.zeros((), dtype=dtype))


def _keep_from_block(src, dst, block0, h, p, seed, offset):
    """dropout_reference.keep for the heads 4 * block0 .. 4 * block0 + h - 1: the same counters, blocks block0, block0 + 1, ..."""
    import numpy as np
    if block0 == 0:
        return R.keep(src, dst, h, p, seed, offset)
    src, dst = np.asarray(src, dtype=np.uint64), np.asarray(dst, dtype=np.uint64)
    assert 0 <= p < 1 and 0 <= int(seed) < 2 ** 63 and 0 <= offset < 2 ** 32 and 0 <= block0 + (h + 3) // 4 <= 2 ** 32
    out = np.empty((src.shape[0], h), dtype=bool)
    for b in range((h + 3) // 4):
        w = R.philox4x32_10((src, dst, block0 + b, offset), (int(seed) & R.MASK, int(seed) >> 32))
        n = min(4, h - 4 * b)
        out[:, 4 * b:4 * b + n] = w[:, :n].astype(np.uint64) >= np.uint64(R.threshold(p))
    return out


def _three(x):
    return x if x.dim() == 3 else x[:, None, :]


def scores(src, dst, Q, K):
    """(E, h) scores; Q (n_q, d) / (n_q, h, d), K likewise"""
    return (_three(Q)[src] * _three(K)[dst]).sum(-1)


def softmax_stats(src, n_q, s):
    """(m, l) per (row, head) of the scores s (E, h): m = max(-1e9, row max), l = sum exp(s - m); rows without edges
    read (-1e9, 0)"""
    h = s.size(1)
    m = torch.full((n_q, h), -1e9, dtype=s.dtype).scatter_reduce(0, src[:, None].expand(-1, h), s.detach(), "amax")
    l = torch.zeros((n_q, h), dtype=s.dtype).index_add(0, src, torch.exp(s - m[src]))
    return m, l


def attention_dropout(src, dst, n_q, Q, K, V, p, seed, offset=0, head0=0):
    """o (n_q[, h], d), autograd-able.  p = 0 is the undropped layer."""
    s = scores(src, dst, Q, K)
    h = s.size(1)
    m, l = softmax_stats(src, n_q, s)
    a = torch.exp(s - m[src]) / l[src]
    if p > 0:
        a = a * head_multipliers(src.numpy(), dst.numpy(), head0, h, p, seed, offset, s.dtype)
    o = torch.zeros((n_q, h, V.size(-1)), dtype=V.dtype).index_add(0, src, a[..., None] * _three(V)[dst])
    return o if V.dim() == 3 else o[:, 0, :]


def reference_step(src, dst, n_q, Q, K, V, dO, p, seed, offset=0, head0=0):
    """-> dict(o, dQ, dK, dV, stats) in float64 from autograd; stats (n_q, h, 2) = (m, 1 / l), (0, 0) for empty rows"""
    q, k, v = (x.double().clone().requires_grad_(True) for x in (Q, K, V))
    o = attention_dropout(src, dst, n_q, q, k, v, p, seed, offset, head0)
    o.backward(dO.double())
    m, l = softmax_stats(src, n_q, scores(src, dst, q.detach(), k.detach()))
    has = l > 0
    stats = torch.stack([torch.where(has, m, torch.zeros_like(m)), torch.where(has, 1 / l, torch.zeros_like(l))], -1)
    return dict(o=o.detach(), dQ=q.grad, dK=k.grad, dV=v.grad, stats=stats)


def restated(src, dst, n_q, n_k, Q, K, V, dO, mult):
    """The step as the kernels compute it, mult = m (E, h): a from the statistics of the undropped scores, o of the
    dropped weights, D_i = <dO_i, o_i>, da = m <dO_i, V_j>, ds = a (da - D_i), then the three sums.
    -> (o, D, dQ, dK, dV) with (n, h, d) operands"""
    Q, K, V, dO = (_three(x) for x in (Q, K, V, dO))
    s = (Q[src] * K[dst]).sum(-1)
    m, l = softmax_stats(src, n_q, s)
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
    return o, D, dQ, dK, dV
