"""Plain float64 statement of the fused GAT layer as its bfloat16 form computes it: the forward from
(src, dst, el, er, V, slope, multipliers) and the backward as a function of the o it is GIVEN (D_i = <dO_i, o_i> from that
o), by the explicit formulas of 4.5c and 4.5d.  el / er are (n, h), V / o / dO (n, h, d); mult is the (E, h) tensor of
dropout_reference.multipliers, or None."""
import torch


def _weights(src, dst, n_src, el, er, slope, mult):
    """-> z (E, h), the undropped a, a * m, and the row statistics m, 1 / l (n_src, h)"""
    z = el.double()[src] + er.double()[dst]
    s = torch.where(z > 0, z, z * slope)
    idx = src[:, None].expand_as(s)
    m = torch.full((n_src, s.size(1)), -1e9, dtype=torch.float64).scatter_reduce(0, idx, s, "amax")
    ex = torch.exp(s - m[src])
    l = torch.zeros_like(m).index_add(0, src, ex)
    linv = torch.where(l > 0, 1 / l, torch.zeros_like(l))
    a = ex * linv[src]
    return z, a, a if mult is None else a * mult.double(), m, linv


def forward(src, dst, n_src, el, er, V, slope, mult=None):
    """-> o (n_src, h, d), m, 1 / l; rows without edges: o = 0, (m, 1 / l) = (-1e9, 0)"""
    _, _, am, m, linv = _weights(src, dst, n_src, el, er, slope, mult)
    o = torch.zeros((n_src,) + tuple(V.shape[1:]), dtype=torch.float64).index_add(0, src, am[..., None] * V.double()[dst])
    return o, m, linv


def backward(src, dst, el, er, V, o, dO, slope, mult=None):
    """-> del, der, dV for the o given: da = m <dO_i, V_j>, ds = a (da - D_i), dz = ds (z > 0 ? 1 : slope)"""
    n_src, n_dst = el.size(0), er.size(0)
    z, a, am, _, _ = _weights(src, dst, n_src, el, er, slope, mult)
    dO, V = dO.double(), V.double()
    D = (dO * o.double()).sum(-1)
    da = (dO[src] * V[dst]).sum(-1)
    if mult is not None:
        da = da * mult.double()
    ds = a * (da - D[src])
    dz = torch.where(z > 0, ds, ds * slope)
    d_el = torch.zeros((n_src, z.size(1)), dtype=torch.float64).index_add(0, src, dz)
    d_er = torch.zeros((n_dst, z.size(1)), dtype=torch.float64).index_add(0, dst, dz)
    dV = torch.zeros_like(V).index_add(0, dst, am[..., None] * dO[src])
    return d_el, d_er, dV
