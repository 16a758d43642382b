"""Plain float64 reference of the fused attention step on bfloat16 operands, over the graph's COO edges:
s = <Q_i, K_j>, m = max(-1e9, max_j s), a = exp(s - m) / l, o = sum_j a V_j; the backward is a function of the `o` it is
given, D = <dO, o>, as the C ABI defines it.  Operands are (n, h, d) tensors, converted exactly with .double().
dtype=torch.float32 evaluates the same lines in fp32: the "plain torch" evaluation the battery's host tier measures
(tests/test_attention_bf16_fuzz_host.py); every expected value is the float64 one."""
import torch


def forward(src, dst, n_q, Q, K, V, dtype=torch.float64):
    """-> o (n_q, h, d), m (n_q, h), 1 / l (n_q, h); rows without edges: o = 0, 1 / l = 0 (m is then meaningless)"""
    Q, K, V = Q.to(dtype), K.to(dtype), V.to(dtype)
    s = (Q[src] * K[dst]).sum(-1)
    idx = src[:, None].expand_as(s)
    m = torch.full((n_q, s.size(1)), float("-inf"), dtype=dtype).scatter_reduce(0, idx, s, "amax").clamp(min=-1e9)
    p = torch.exp(s - m[src])
    l = torch.zeros_like(m).index_add_(0, src, p)
    linv = torch.where(l > 0, 1 / l, torch.zeros_like(l))
    a = p * linv[src]
    o = torch.zeros_like(Q).index_add_(0, src, a[..., None] * V[dst])
    return o, m, linv, a


def backward(src, dst, Q, K, V, o, dO, dtype=torch.float64):
    """-> dQ, dK, dV for the output gradient dO and the saved output o (as the op returned it)"""
    a = forward(src, dst, Q.size(0), Q, K, V, dtype)[3]
    Q, K, V, o, dO = (x.to(dtype) for x in (Q, K, V, o, dO))
    ds = a * ((dO[src] * V[dst]).sum(-1) - (dO * o).sum(-1)[src])
    dQ = torch.zeros_like(Q).index_add_(0, src, ds[..., None] * K[dst])
    dK = torch.zeros_like(K).index_add_(0, dst, ds[..., None] * Q[src])
    dV = torch.zeros_like(V).index_add_(0, dst, a[..., None] * dO[src])
    return dQ, dK, dV
