"""Shared by test_fused_gatv2_host.py (no GPU) and test_fused_gatv2.py (GPU): the graphs and inputs of the fused GATv2
layer's tests, its float64 reference (autograd through gatv2_reference.gatv2_layer with V=None, one head at a time so
that no temporary exceeds (E, d) values), the backward restated as the kernels compute it, and the bounds:

  o, stats, dxl, dxr : rtol = 1e-4, atol = 1e-5 against float64 (1e-10 / 1e-10 in fp64)
  datt               : |err| <= K * S[k, c],  S = sum_e |ds[e, k] * LeakyReLU(z[e, k, c])| with ds from the reference
                       (with_scores=True and retain_grad()); K = 1e-6 (1e-12 in fp64)
"""
import functools

import torch
import torch.nn.functional as F

from gatv2_reference import gatv2_datt_scale, gatv2_layer
from util import random_graph

FAST = [(1, 64), (2, 32), (2, 64), (4, 16), (4, 32), (4, 64), (8, 8), (8, 16), (8, 32)]
TOL32, TOL64 = dict(rtol=1e-4, atol=1e-5), dict(rtol=1e-10, atol=1e-10)
K32, K64 = 1e-6, 1e-12
FLOOR = -1e9
# slots per batch of the forward at the three row widths (Gv2AttnCfg::SB_FWD = 16 / NV) and the long-segment bound
EDGE_ROWS = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 1024, 1025, 2049, 5000)


def node_shape(n, h, d):
    return (n, d) if h == 1 else (n, h, d)


def inputs(g, h, d, seed, dtype=torch.float32, kind="normal", slope=0.2):
    """xl, xr, dO standard normal, att normal / sqrt(d).  kind "ties": xl, xr small integers with xr = -xl on shared
    ids (z == 0 exactly on many elements).  kind "large": every row of xl is moved along +sign(att) (even rows) or
    -sign(att) (odd rows), far enough for max |s| = 56 at `slope` up to the O(1) spread of the scores inside a row:
    exp(s) without the running maximum overflows or vanishes, while s - m stays O(1), so the softmax keeps several
    weights per row and the gradients stay as well conditioned as with the plain inputs (scaling all scores instead
    leaves one weight per row and a da - D that cancels: torch's own fp32 result then misses rtol = 1e-4)."""
    gen = torch.Generator().manual_seed(seed)
    if kind == "ties":
        xl = torch.randint(-2, 3, node_shape(g.n_src, h, d), generator=gen).to(dtype)
        xr = torch.randint(-2, 3, node_shape(g.n_dst, h, d), generator=gen).to(dtype)
        m = min(g.n_src, g.n_dst)
        xr[:m] = -xl[:m]
    else:
        xl = torch.randn(node_shape(g.n_src, h, d), generator=gen, dtype=dtype)
        xr = torch.randn(node_shape(g.n_dst, h, d), generator=gen, dtype=dtype)
    att = torch.randn(node_shape(1, h, d)[1:], generator=gen, dtype=dtype) / d ** 0.5
    if kind == "large":
        sign = torch.where(torch.arange(g.n_src) % 2 == 0, 1.0, -1.0).to(dtype).view(-1, *([1] * (xl.dim() - 1)))
        push = att.sign() * sign * (100.0 / float(att.abs().sum(-1).min()))
        s = (F.leaky_relu((xl + push).double()[g.src] + xr.double()[g.dst], slope) * att.double()).sum(-1)
        xl = xl + push * (56.0 / float(s.abs().max()))       # LeakyReLU is positively homogeneous: |s| scales with it
    dO = torch.randn(node_shape(g.n_src, h, d), generator=gen, dtype=dtype)
    return xl, xr, att, dO


def _heads(t):
    if t.dim() == 2:
        return [lambda x: x], lambda xs: xs[0]
    return [(lambda x, k=k: x[:, k]) for k in range(t.size(1))], lambda xs: torch.stack(xs, 1)


def reference(g, xl, xr, att, dO, slope, dtype=torch.float64):
    """(o, stats, dxl, dxr, datt, S, s) by autograd in `dtype`, one head at a time: stats (n_src, h, 2) = (m, 1 / l)
    with (-1e9, 0) on rows without edges, S the scale datt's error is measured against (always float64), s the scores."""
    sel, join = _heads(xl)
    one = xl.dim() == 2
    outs = [[] for _ in range(7)]
    for k, head in enumerate(sel):
        att_k = att if one else att[k]
        r = [t.to(dtype).clone().requires_grad_(True) for t in (head(xl), head(xr), att_k)]
        o, s = gatv2_layer(g.src, g.dst, g.n_src, r[0], r[1], r[2], slope, None, with_scores=True)
        s.retain_grad()
        o.backward(head(dO).to(dtype))
        sd = s.detach()
        m = torch.full((g.n_src,), FLOOR, dtype=dtype).scatter_reduce(0, g.src, sd, "amax")
        den = torch.zeros(g.n_src, dtype=dtype).index_add(0, g.src, torch.exp(sd - m[g.src]))
        il = torch.where(den > 0, 1 / den, torch.zeros_like(den))
        S = gatv2_datt_scale(g.src, g.dst, head(xl), head(xr), s.grad, slope)
        for lst, t in zip(outs, (o.detach(), torch.stack([m, il], -1), r[0].grad, r[1].grad, r[2].grad, S, sd)):
            lst.append(t)
    stack0 = (lambda xs: xs[0]) if one else (lambda xs: torch.stack(xs, 0))
    return (join(outs[0]), torch.stack(outs[1], 1), join(outs[2]), join(outs[3]), stack0(outs[4]), stack0(outs[5]),
            join(outs[6]))


def restated(src, dst, n_l, xl, xr, att, dO, slope):
    """The op as the kernels compute it (include/graphop_hip.h), in the tensors' dtype: stats, o, D, da, ds, then the three
    sums.  xl (n_l, h, d), xr (n_r, h, d), att (h, d), dO (n_l, h, d) -> (o, stats, dxl, dxr, datt)."""
    h = xl.size(1)
    z = xl[src] + xr[dst]                                             # (E, h, d)
    lz = F.leaky_relu(z, slope)
    s = (lz * att).sum(-1)                                            # (E, h)
    m = torch.full((n_l, h), FLOOR, dtype=s.dtype).scatter_reduce(0, src[:, None].expand(-1, h), s, "amax")
    ex = torch.exp(s - m[src])
    lsum = torch.zeros((n_l, h), dtype=s.dtype).index_add(0, src, ex)
    inv_l = torch.where(lsum > 0, 1 / lsum, torch.zeros_like(lsum))
    a = ex * inv_l[src]
    o = torch.zeros_like(xl).index_add(0, src, a[..., None] * xr[dst])
    D = (dO * o).sum(-1)
    da = (dO[src] * xr[dst]).sum(-1)
    ds = a * (da - D[src])
    t = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))     # a tie takes the slope
    dxl = att * torch.zeros_like(xl).index_add(0, src, ds[..., None] * t)
    dxr = torch.zeros_like(xr).index_add(0, dst, ds[..., None] * att * t + a[..., None] * dO[src])
    datt = (ds[..., None] * lz).sum(0)
    return o, torch.stack([m, inv_l], -1), dxl, dxr, datt


def ratio(got, want, tol=TOL32):
    """max |got - want| / (atol + rtol * |want|): <= 1 is inside the bound"""
    want = want.double()
    if want.numel() == 0:
        return 0.0
    return float(((got.detach().cpu().double() - want).abs() / (tol["atol"] + tol["rtol"] * want.abs())).max())


def datt_ratio(got, want, S):
    """max |got - want| / S: <= K is inside the bound"""
    return float(((got.detach().cpu().double() - want.double()).abs() / S.clamp_min(1e-300)).max())


# ---- the graphs of the GPU tests ---------------------------------------------------------------------------------
def irregular_graph(chunk_size):
    """a fifth of the rows empty, one hub row above the 1024-slot long-segment bound"""
    return random_graph(300, 300, 3000, seed=17 + chunk_size, chunk_size=chunk_size, zero_rows=0.2, hub=1500)


@functools.lru_cache(maxsize=None)
def edge_rows_graph():
    """Rows of exactly EDGE_ROWS slots (1, SB - 1, SB, SB + 1 for SB = 4, 8, 16; 1024, 1025, 2049, 5000 around the
    long-segment bound) between empty rows and rows of 2 and 40 slots, in random order; rectangular."""
    from test_gat_launch_geometry import _from_lengths
    gen = torch.Generator().manual_seed(23)
    lens = torch.tensor(list(EDGE_ROWS) + [0, 0, 0, 2, 2, 40, 40, 40, 0])
    assert int((lens > 0).sum()) % 16 != 0
    return _from_lengths(lens[torch.randperm(len(lens), generator=gen)], gen, 32)


def slopes_graph():
    return random_graph(200, 350, 4000, seed=7, chunk_size=8, hub=300)
