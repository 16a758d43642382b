"""Shared by test_gatv2_dropout_host.py (no GPU) and test_gatv2_dropout.py (GPU): the fused GATv2 layer with attention
dropout (include/graphop_hip.h) as a float64 reference and restated as the kernels compute it.  Nothing
here is new: the scores are gatv2_reference.gatv2_scores, the multipliers dropout_reference.multipliers (i = src indexes
xl / o, j = dst indexes xr), graphs, inputs and ratios those of fused_gatv2_reference, and the bounds are

  o, stats, dxl, dxr : rtol = 1e-4, atol = 1e-5 / (1 - p) against float64 (every term is scaled by 1 / (1 - p): the rule
                       of test_gat_dropout.py); 1e-10 / 1e-10 in fp64
  datt               : |err| <= K * S[k, c],  S = gatv2_datt_scale(..., ds of this reference, ...); K = 1e-6 (1e-12 in fp64)
"""
import torch
import torch.nn.functional as F

import dropout_reference as DR
import fused_gatv2_reference as R
from gatv2_reference import gatv2_datt_scale, gatv2_scores

FLOOR = R.FLOOR


def tol(dtype, p):
    if dtype == torch.float32:
        return dict(rtol=1e-4, atol=1e-5 / (1 - p)), R.K32
    return dict(R.TOL64), R.K64


def layer(src, dst, n_out, xl, xr, att, negative_slope, mult):
    """One head: o[i] = sum_j a_ij m_ij xr[j] with a the row softmax of the undropped scores; xl (n_l, d), xr (n_r, d),
    att (d), mult (E).  -> (o, s), s the scores (retain_grad() on it gives the layer's ds).  Autograd-able."""
    s = gatv2_scores(src, dst, xl, xr, att, negative_slope)
    m = torch.full((n_out,), float("-inf"), dtype=s.dtype).scatter_reduce(0, src, s.detach(), "amax")
    ex = torch.exp(s - m[src])
    den = torch.zeros(n_out, dtype=s.dtype).index_add(0, src, ex)
    a = ex / den[src] * mult
    return torch.zeros((n_out, xr.size(-1)), dtype=xr.dtype).index_add(0, src, a[:, None] * xr[dst]), s


def reference(g, xl, xr, att, dO, slope, p, seed, offset, dtype=torch.float64):
    """(o, stats, dxl, dxr, datt, S) by autograd in `dtype`, one head at a time with that head's multipliers (as
    fused_gatv2_reference.reference): stats (n_src, h, 2) = (m, 1 / l) of the undropped scores, S the scale datt's
    error is measured against (always float64)."""
    sel, join = R._heads(xl)
    one = xl.dim() == 2
    mult = DR.multipliers(g.src.numpy(), g.dst.numpy(), len(sel), p, seed, offset, dtype)
    outs = [[] for _ in range(6)]
    for k, head in enumerate(sel):
        r = [t.to(dtype).clone().requires_grad_(True) for t in (head(xl), head(xr), att if one else att[k])]
        o, s = layer(g.src, g.dst, g.n_src, r[0], r[1], r[2], slope, mult[:, k])
        s.retain_grad()
        o.backward(head(dO).to(dtype))
        sd = s.detach()
        m = torch.full((g.n_src,), FLOOR, dtype=dtype).scatter_reduce(0, g.src, sd, "amax")
        den = torch.zeros(g.n_src, dtype=dtype).index_add(0, g.src, torch.exp(sd - m[g.src]))
        il = torch.where(den > 0, 1 / den, torch.zeros_like(den))
        S = gatv2_datt_scale(g.src, g.dst, head(xl), head(xr), s.grad, slope)
        for lst, t in zip(outs, (o.detach(), torch.stack([m, il], -1), r[0].grad, r[1].grad, r[2].grad, S)):
            lst.append(t)
    stack0 = (lambda xs: xs[0]) if one else (lambda xs: torch.stack(xs, 0))
    return join(outs[0]), torch.stack(outs[1], 1), join(outs[2]), join(outs[3]), stack0(outs[4]), stack0(outs[5])


def restated(src, dst, n_l, xl, xr, att, dO, slope, mult):
    """The op as the kernels compute it (include/graphop_hip.h), in the tensors' dtype, mult = m (E, h): stats of the
    undropped scores, o of the dropped weights, D = <dO, o>, da = m <dO, xr>, ds, then the three sums.  xl (n_l, h, d),
    xr (n_r, h, d), att (h, d), dO (n_l, h, d) -> (o, stats, dxl, dxr, datt)."""
    h = xl.size(1)
    z = xl[src] + xr[dst]                                             # (E, h, d)
    lz = F.leaky_relu(z, slope)
    s = (lz * att).sum(-1)                                            # (E, h)
    m = torch.full((n_l, h), FLOOR, dtype=s.dtype).scatter_reduce(0, src[:, None].expand(-1, h), s, "amax")
    ex = torch.exp(s - m[src])
    lsum = torch.zeros((n_l, h), dtype=s.dtype).index_add(0, src, ex)
    inv_l = torch.where(lsum > 0, 1 / lsum, torch.zeros_like(lsum))
    a = ex * inv_l[src]
    am = a * mult
    o = torch.zeros_like(xl).index_add(0, src, am[..., None] * xr[dst])
    D = (dO * o).sum(-1)
    da = mult * (dO[src] * xr[dst]).sum(-1)
    ds = a * (da - D[src])
    t = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))     # a tie takes the slope
    dxl = att * torch.zeros_like(xl).index_add(0, src, ds[..., None] * t)
    dxr = torch.zeros_like(xr).index_add(0, dst, ds[..., None] * att * t + am[..., None] * dO[src])
    datt = (ds[..., None] * lz).sum(0)
    return o, torch.stack([m, inv_l], -1), dxl, dxr, datt
