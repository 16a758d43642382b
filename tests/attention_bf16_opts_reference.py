"""Plain float64 reference of the bfloat16 fused attention step with attention dropout and a per-edge score bias
(DESIGN.md 4.5w), over the graph's COO edges IN EDGE-ID ORDER (edge e = (src[e], dst[e]); b and db are indexed by e):
  s = <Q_i, K_j> + b[e],  m = max(-1e9, max s),  a = exp(s - m) / l  (l sums the undropped exp),  o = sum_e a mult V_j
  D = <dO, o> from the o it is given,  da = mult <dO_i, V_j>,  ds = a (da - D) = db,  dQ, dK from ds,  dV from a mult dO.
mult (E, h) comes from attention_dropout_reference.head_multipliers for the global heads head0 .. head0 + h - 1; None or
p == 0: ones.  Operands are (n, h, d) tensors and b (E, h), converted exactly with .to(dtype); dtype=torch.float32
evaluates the same lines in fp32, as in attention_bf16_reference.py.  Every expected value is the float64 one."""
import torch

from attention_dropout_reference import head_multipliers


def multipliers(src, dst, h, p, seed, offset=0, head0=0, dtype=torch.float64):
    if not p:
        return torch.ones((src.numel(), h), dtype=dtype)
    return head_multipliers(src.numpy(), dst.numpy(), head0, h, p, seed, offset).to(dtype)


def forward(src, dst, n_q, Q, K, V, b=None, mult=None, dtype=torch.float64):
    """-> o (n_q, h, d), m (n_q, h), 1 / l (n_q, h), a (E, h) undropped; rows without edges: o = 0, 1 / l = 0"""
    Q, K, V = Q.to(dtype), K.to(dtype), V.to(dtype)
    s = (Q[src] * K[dst]).sum(-1)
    if b is not None:
        s = s + b.to(dtype)
    idx = src[:, None].expand_as(s)
    m = torch.full((n_q, s.size(1)), float("-inf"), dtype=dtype).scatter_reduce(0, idx, s, "amax").clamp(min=-1e9)
    p = torch.exp(s - m[src])
    l = torch.zeros_like(m).index_add_(0, src, p)
    linv = torch.where(l > 0, 1 / l, torch.zeros_like(l))
    a = p * linv[src]
    w = a if mult is None else a * mult.to(dtype)
    o = torch.zeros_like(Q).index_add_(0, src, w[..., None] * V[dst])
    return o, m, linv, a


def backward(src, dst, Q, K, V, o, dO, b=None, mult=None, dtype=torch.float64):
    """-> dQ, dK, dV, db for the output gradient dO and the saved output o (as the op returned it)"""
    a = forward(src, dst, Q.size(0), Q, K, V, b, mult, dtype)[3]
    Q, K, V, o, dO = (x.to(dtype) for x in (Q, K, V, o, dO))
    mult = torch.ones_like(a) if mult is None else mult.to(dtype)
    ds = a * (mult * (dO[src] * V[dst]).sum(-1) - (dO * o).sum(-1)[src])
    dQ = torch.zeros_like(Q).index_add_(0, src, ds[..., None] * K[dst])
    dK = torch.zeros_like(K).index_add_(0, dst, ds[..., None] * Q[src])
    dV = torch.zeros_like(V).index_add_(0, dst, (a * mult)[..., None] * dO[src])
    return dQ, dK, dV, ds
