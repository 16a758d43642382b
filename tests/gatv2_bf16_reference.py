"""Plain float64 statement of the fused GATv2 layer as its bfloat16 form computes it: the forward from
(src, dst, xl, xr, att, slope, multipliers) and the backward as a function of the o it is GIVEN (D_i = <dO_i, o_i> from
that o), by the explicit formulas of fused_gatv2_reference.restated plus the (E, h) multipliers of
dropout_reference.multipliers (None: no dropout).  xl / o / dO are (n_l, h, d), xr (n_r, h, d), att (h, d).  dt = torch.float32 evaluates the same lines in fp32
(test_gatv2_attention_bf16_host.py measures how much of each bound that alone uses)."""
import torch

FLOOR = -1e9


def _weights(src, dst, n_l, xl, xr, att, slope, mult, dt):
    """-> z (E, h, d), LeakyReLU(z), the undropped a (E, h), a * m, and the row statistics m, 1 / l (n_l, h)"""
    z = xl.to(dt)[src] + xr.to(dt)[dst]
    lz = torch.clamp(z, min=0) + slope * torch.clamp(z, max=0)
    s = (lz * att.to(dt)).sum(-1)
    m = torch.full((n_l, s.size(1)), FLOOR, dtype=dt).scatter_reduce(0, src[:, None].expand_as(s), s, "amax")
    ex = torch.exp(s - m[src])
    l = torch.zeros_like(m).index_add(0, src, ex)
    linv = torch.where(l > 0, 1 / l, torch.zeros_like(l))
    a = ex * linv[src]
    return z, lz, a, a if mult is None else a * mult.to(dt), m, linv


def forward(src, dst, n_l, xl, xr, att, slope, mult=None, dt=torch.float64):
    """-> o (n_l, h, d), m, 1 / l; rows without edges: o = 0, (m, 1 / l) = (-1e9, 0)"""
    _, _, _, am, m, linv = _weights(src, dst, n_l, xl, xr, att, slope, mult, dt)
    o = torch.zeros(xl.shape, dtype=dt).index_add(0, src, am[..., None] * xr.to(dt)[dst])
    return o, m, linv


def backward(src, dst, xl, xr, att, o, dO, slope, mult=None, dt=torch.float64):
    """-> dxl, dxr, datt, S for the o given: da = m <dO_i, xr_j>, ds = a (da - D_i), t = (z > 0 ? 1 : slope);
    S[k, c] = sum_e |ds LeakyReLU(z)|, the scale datt's error is measured against"""
    z, lz, a, am, _, _ = _weights(src, dst, xl.size(0), xl, xr, att, slope, mult, dt)
    dO, xr, att = dO.to(dt), xr.to(dt), att.to(dt)
    D = (dO * o.to(dt)).sum(-1)
    da = (dO[src] * xr[dst]).sum(-1)
    if mult is not None:
        da = da * mult.to(dt)
    ds = a * (da - D[src])
    t = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))          # a tie takes the slope
    dxl = att * torch.zeros(xl.shape, dtype=dt).index_add(0, src, ds[..., None] * t)
    dxr = torch.zeros_like(xr).index_add(0, dst, ds[..., None] * att * t + am[..., None] * dO[src])
    return dxl, dxr, (ds[..., None] * lz).sum(0), (ds[..., None] * lz).abs().sum(0)
