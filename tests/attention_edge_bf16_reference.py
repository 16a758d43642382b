"""Plain float64 reference of the bfloat16 fused attention step with edge features, over the graph's COO
edges IN EDGE-ID ORDER (edge e = (src[e], dst[e]); xe and dxe are indexed by e):
  s = <Q_i, K_j + xe[e]>,  m = max(-1e9, max s),  a = exp(s - m) / l  (l sums the undropped exp),  o = sum_e a mult (V_j + xe[e])
  D = <dO, o> from the o it is given,  da = mult <dO_i, V_j + xe[e]>,  ds = a (da - D),  dQ = sum ds (K_j + xe[e]),
  dK = sum ds Q_i,  dV = sum a mult dO_i,  dxe[e] = ds Q_i + a mult dO_i.
mult (E, h) comes from attention_bf16_opts_reference.multipliers (ones at p == 0).  Operands are (n, h, d) tensors and xe
(E, h, d), converted exactly with .to(dtype); dtype=torch.float32 evaluates the same lines in fp32.  Every expected value
is the float64 one."""
import torch

from attention_bf16_opts_reference import multipliers          # noqa: F401 (the family's multipliers, re-exported)


def _weights(src, dst, n_q, Q, K, xe):
    s = (Q[src] * (K[dst] + xe)).sum(-1)
    idx = src[:, None].expand_as(s)
    m = torch.full((n_q, s.size(1)), float("-inf"), dtype=s.dtype).scatter_reduce(0, idx, s, "amax").clamp(min=-1e9)
    p = torch.exp(s - m[src])
    l = torch.zeros_like(m).index_add_(0, src, p)
    linv = torch.where(l > 0, 1 / l, torch.zeros_like(l))
    return p * linv[src], m, linv


def forward(src, dst, n_q, Q, K, V, xe, mult, dtype=torch.float64):
    """-> o (n_q, h, d), m (n_q, h), 1 / l (n_q, h); rows without edges: o = 0, 1 / l = 0"""
    Q, K, V, xe, mult = (x.to(dtype) for x in (Q, K, V, xe, mult))
    a, m, linv = _weights(src, dst, n_q, Q, K, xe)
    o = torch.zeros_like(Q).index_add_(0, src, (a * mult)[..., None] * (V[dst] + xe))
    return o, m, linv


def backward(src, dst, Q, K, V, xe, o, dO, mult, dtype=torch.float64):
    """-> dQ, dK, dV, dxe for the output gradient dO and the saved output o (as the op returned it)"""
    Q, K, V, xe, o, dO, mult = (x.to(dtype) for x in (Q, K, V, xe, o, dO, mult))
    a = _weights(src, dst, Q.size(0), Q, K, xe)[0]
    ds = a * (mult * (dO[src] * (V[dst] + xe)).sum(-1) - (dO * o).sum(-1)[src])
    am = a * mult
    dQ = torch.zeros_like(Q).index_add_(0, src, ds[..., None] * (K[dst] + xe))
    dK = torch.zeros_like(K).index_add_(0, dst, ds[..., None] * Q[src])
    dV = torch.zeros_like(V).index_add_(0, dst, am[..., None] * dO[src])
    return dQ, dK, dV, ds[..., None] * Q[src] + am[..., None] * dO[src]
