"""Pure-torch reference of the GATv2 attention scores and of the GATv2 attention layer built on them
(graphop.gatv2_scores_forward / _backward, functions.GATv2Scores, functions.gatv2_attention_step).  CPU, autograd-able."""
import torch
import torch.nn.functional as F


def gatv2_scores(src, dst, xl, xr, att, negative_slope):
    """s[e, k] = sum_c att[k, c] * LeakyReLU(xl[src[e], k, c] + xr[dst[e], k, c]): (E) for 2-D xl / xr and 1-D att,
    else (E, h)."""
    return (F.leaky_relu(xl[src] + xr[dst], negative_slope) * att).sum(-1)


def gatv2_datt_scale(src, dst, xl, xr, dy, negative_slope):
    """S[k, c] = sum_e |dy[e, k] * LeakyReLU(z[e, k, c])| in float64, in att's shape: the magnitude a rounding error of
    datt (a sum of E terms of mixed sign) is measured against."""
    z = F.leaky_relu(xl.double()[src] + xr.double()[dst], negative_slope)
    return (dy.double().unsqueeze(-1) * z).abs().sum(0)


def gatv2_layer(src, dst, n_out, xl, xr, att, negative_slope, V=None, with_scores=False):
    """o[i] = sum_j a_ij V[j], a = softmax over the edges (i, j) of row i of the GATv2 scores; V=None aggregates xr (the
    GATv2Conv convention).  The segment softmax of gat_reference.gat_layer: max by scatter_reduce, sums by index_add.
    with_scores: -> (o, s), s the score tensor o was computed from (retain_grad() on it gives the layer's ds)."""
    s = gatv2_scores(src, dst, xl, xr, att, negative_slope)
    V = xr if V is None else V
    s2 = s if s.dim() == 2 else s[:, None]
    h = s2.size(1)
    idx = src[:, None].expand(-1, h)
    m = torch.full((n_out, h), float("-inf"), dtype=s2.dtype).scatter_reduce(0, idx, s2.detach(), "amax")
    ex = torch.exp(s2 - m[src])
    den = torch.zeros((n_out, h), dtype=s2.dtype).index_add(0, src, ex)
    a = ex / den[src]
    V3 = V if V.dim() == 3 else V[:, None, :]
    o = torch.zeros((n_out, h, V3.size(-1)), dtype=V.dtype).index_add(0, src, a[..., None] * V3[dst])
    o = o if V.dim() == 3 else o[:, 0, :]
    return (o, s) if with_scores else o
