"""Pure-torch reference of the fused GATv2 layer with edge features (graphop.gatv2_attention_dropout_forward / _backward
with xe, functions.FusedGATv2EdgeAttention), and the inputs its CPU and GPU tests share.  CPU, autograd-able.

For edge e = (src[e], dst[e]), per head k:
  z = (xl[src] + xr[dst]) + xe,  s = sum_c att[k, c] LeakyReLU(z),  a = row-softmax(s),  o[i] = sum_e a_e m_e xr[dst[e]]
(src, dst) are in EDGE-ID order: edge e owns xe[e].  gat_edge_reference.permute_edge_ids renumbers a graph's edges, so
that a slot's position and its edge id differ.  The reference goes one head at a time, so that no temporary exceeds
(E, d) values.  Bounds (none new): rtol 1e-4 / atol 1e-5 for fp32 against float64 on o, dxl, dxr, dxe (atol / (1 - p)
with dropout), |datt err| <= 1e-6 S with S = sum_e |ds_e LeakyReLU(z_e)| (fused_gatv2_reference.datt_ratio), 1e-10 /
1e-12 S in fp64."""
import torch
import torch.nn.functional as F

import dropout_reference as R
from fused_gatv2_reference import FLOOR, K32, K64, TOL32, TOL64, datt_ratio, ratio
from gat_edge_reference import hub_row, permute_edge_ids
from util import random_graph

NAMES = ("o", "dxl", "dxr", "dxe", "datt")
FAST = [(1, 64), (2, 32), (2, 64), (4, 16), (4, 32), (4, 64), (8, 8), (8, 16), (8, 32)]


def node_shape(n, h, d):
    return (n, d) if h == 1 else (n, h, d)


def _head(t, k):
    """head k of a per-node or per-edge operand (n[, h], d), or of att ([h,] d), given the operand's one-head rank"""
    return t[:, k] if t.dim() == 3 else t


def layer_head(src, dst, n_out, xl, xr, xe, att, slope, mult=None):
    """one head: xl (n_src, d), xr (n_dst, d), xe (E, d), att (d), mult (E) -> (o (n_out, d), s (E))"""
    z = (xl[src] + xr[dst]) + xe
    s = (F.leaky_relu(z, slope) * att).sum(-1)
    m = torch.full((n_out,), float("-inf"), dtype=s.dtype).scatter_reduce(0, src, s.detach(), "amax")
    ex = torch.exp(s - m[src])
    a = ex / torch.zeros(n_out, dtype=s.dtype).index_add(0, src, ex)[src]
    if mult is not None:
        a = a * mult
    return torch.zeros((n_out, xr.size(-1)), dtype=xr.dtype).index_add(0, src, a[:, None] * xr[dst]), s


def reference(src, dst, n_src, xl, xr, xe, att, dO, slope, p=0.0, seed=0, offset=0, dtype=torch.float64):
    """(o, dxl, dxr, dxe, datt, S, stats) by autograd through layer_head evaluated in `dtype`, one head at a time.  S is
    the scale datt's error is measured against (float64), stats (n_src, h, 2) = (m, 1 / l) of the undropped scores with
    (-1e9, 0) on rows without edges."""
    one = xl.dim() == 2
    h = 1 if one else xl.size(1)
    mult = R.multipliers(src.numpy(), dst.numpy(), h, p, seed, offset, dtype).reshape(-1, h) if p > 0 else None
    outs = [[] for _ in range(7)]
    for k in range(h):
        att_k = att if one else att[k]
        r = [t.detach().to(dtype).clone().requires_grad_(True) for t in (_head(xl, k), _head(xr, k), _head(xe, k), att_k)]
        o, s = layer_head(src, dst, n_src, r[0], r[1], r[2], r[3], slope, None if mult is None else mult[:, k])
        s.retain_grad()
        o.backward(_head(dO, k).to(dtype))
        sd = s.detach()
        m = torch.full((n_src,), FLOOR, dtype=dtype).scatter_reduce(0, src, sd, "amax")
        den = torch.zeros(n_src, dtype=dtype).index_add(0, src, torch.exp(sd - m[src]))
        il = torch.where(den > 0, 1 / den, torch.zeros_like(den))
        z = (r[0].detach().double()[src] + r[1].detach().double()[dst]) + r[2].detach().double()
        S = (s.grad.double()[:, None] * F.leaky_relu(z, slope)).abs().sum(0)
        for lst, t in zip(outs, (o.detach(), r[0].grad, r[1].grad, r[2].grad, r[3].grad, S, torch.stack([m, il], -1))):
            lst.append(t)
    join = (lambda xs: xs[0]) if one else (lambda xs: torch.stack(xs, 1))
    join0 = (lambda xs: xs[0]) if one else (lambda xs: torch.stack(xs, 0))
    return (join(outs[0]), join(outs[1]), join(outs[2]), join(outs[3]), join0(outs[4]), join0(outs[5]),
            torch.stack(outs[6], 1))


def restated(src, dst, n_l, xl, xr, xe, att, dO, slope, mult=None):
    """The op as the kernels compute it, in the tensors' dtype: stats of the undropped scores -> a -> o of the dropped
    weights, D = <dO, o>, da = m <dO, xr>, ds, t, then the sums and dxe = ds att t.  xl (n_l, h, d), xr (n_r, h, d),
    xe (E, h, d), att (h, d), dO (n_l, h, d), mult (E, h) -> (o, dxl, dxr, dxe, datt, stats)."""
    h = xl.size(1)
    if mult is None:
        mult = torch.ones((src.numel(), h), dtype=xl.dtype)
    z = (xl[src] + xr[dst]) + xe
    lz = F.leaky_relu(z, slope)
    s = (lz * att).sum(-1)
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
    dxe = ds[..., None] * att * t
    dxl = att * torch.zeros_like(xl).index_add(0, src, ds[..., None] * t)
    dxr = torch.zeros_like(xr).index_add(0, dst, dxe + am[..., None] * dO[src])
    datt = (ds[..., None] * lz).sum(0)
    return o, dxl, dxr, dxe, datt, torch.stack([m, inv_l], -1)


def inputs(src, dst, n_src, n_dst, h, d, dtype, seed, kind="unit"):
    """(xl, xr, xe, att, dO) on the CPU; att is normal / sqrt(d).  kind:
    "unit"  - unit-scale randn (and, as in "large", no |z| below 1e-4: see the comment below);
    "zero"  - unit-scale randn with xe = 0 (the layer without edge features);
    "ties"  - xl, xr, xe small integers and xe = -(xl[i] + xr[j]) on a random 30 % of the edges: z == 0 exactly there;
    "large" - unit-scale randn, then xe + 50 on every edge of three rows, - 50 on three other rows and + 60 on every
              7th edge of the hub row: |z| up to about 65, the magnitude confined to a few rows."""
    gen = torch.Generator().manual_seed(seed)
    E = src.numel()
    if kind == "ties":
        xl = torch.randint(-2, 3, node_shape(n_src, h, d), generator=gen).to(dtype)
        xr = torch.randint(-2, 3, node_shape(n_dst, h, d), generator=gen).to(dtype)
        xe = torch.randint(-2, 3, node_shape(E, h, d), generator=gen).to(dtype)
        pick = torch.rand(E, generator=gen) < 0.3
        xe[pick] = -(xl[src] + xr[dst])[pick]
    else:
        xl = torch.randn(node_shape(n_src, h, d), generator=gen, dtype=dtype)
        xr = torch.randn(node_shape(n_dst, h, d), generator=gen, dtype=dtype)
        xe = torch.randn(node_shape(E, h, d), generator=gen, dtype=dtype)
        if kind == "large":
            hub = hub_row(src)
            rows = [int(r) for r in torch.unique(src) if int(r) != hub][:6]
            for r in rows[:3]:
                xe[src == r] += 50.0
            for r in rows[3:]:
                xe[src == r] -= 50.0
            on_hub = torch.nonzero(src == hub)[:, 0]
            xe[on_hub[::7]] += 60.0
        elif kind == "zero":
            xe.zero_()
        else:
            assert kind == "unit"
        if kind != "zero":
            # t = (z > 0 ? 1 : slope) jumps at z = 0: an element whose float64 z is closer to 0 than fp32 rounding can
            # take either value in fp32, and dxl, dxr, dxe move by ds att (1 - slope) there.  Such elements (about one in
            # 10^7) are moved away from the jump, so that every comparison measures arithmetic and not the jump.
            near = ((xl.double()[src] + xr.double()[dst]) + xe.double()).abs() < 1e-4
            xe[near] += 0.01
    att = torch.randn(node_shape(1, h, d)[1:], generator=gen, dtype=dtype) / d ** 0.5
    dO = torch.randn(node_shape(n_src, h, d), generator=gen, dtype=dtype)
    return xl, xr, xe, att, dO


def tol(dtype, p=0.0):
    """the bounds on o, dxl, dxr, dxe; with dropout atol / (1 - p): the kept weights are scaled by 1 / (1 - p)"""
    return dict(TOL64) if dtype == torch.float64 else dict(rtol=TOL32["rtol"], atol=TOL32["atol"] / (1 - p))


def worst(got, want, dtype=torch.float32, p=0.0):
    """(max over o, dxl, dxr, dxe of |got - want| / (atol + rtol |want|), |datt err| / (K S)): both <= 1 inside the
    bounds.  got = (o, dxl, dxr, dxe or None, datt); want = reference(...)"""
    t = tol(dtype, p)
    w = max(ratio(x, y, t) for x, y in zip(got[:4], want[:4]) if x is not None and x.numel())
    return w, datt_ratio(got[4], want[4], want[5]) / (K32 if dtype == torch.float32 else K64)


# ---- the graphs and input sets of the GPU tests that compare against the float64 reference -----------------------------
# (name, graph, edge-id permutation seed or None, h, d, input seed, kind, slope, (p, seed, offset) or None)
DROP = (0.3, 2 ** 32 + 12345, 7)         # a seed above 2^32 and a non-zero offset
HUB_GRAPH = {cs: (lambda cs=cs: random_graph(300, 300, 3000, seed=cs, chunk_size=cs, zero_rows=0.2, hub=1500))
             for cs in (3, 32)}
TIES_GRAPH = lambda: random_graph(200, 200, 4000, seed=7, chunk_size=8, zero_rows=0.1, hub=300)   # noqa: E731
RECT_GRAPH = lambda: random_graph(260, 190, 5000, seed=11, chunk_size=8, zero_rows=0.2, hub=500)   # noqa: E731
BIND_GRAPH = lambda: random_graph(500, 400, 8000, seed=6, chunk_size=32, hub=900)   # noqa: E731
# every row and every column inside one chunk: each pass stores plainly and sums in a fixed order, so results repeat
# bit for bit
WHOLE_ROWS_GRAPH = lambda: random_graph(500, 400, 4000, seed=6, chunk_size=32)   # noqa: E731
SLOPES = (0.2, 0.0, -0.1, 1.0)


def parity_cases():
    for cs in (3, 32):
        for h in (1, 2, 3, 4, 8):
            for d in (8, 16, 32):
                yield ("parity cs=%d" % cs, HUB_GRAPH[cs], 100 + cs, h, d, h * 100 + d, "unit", 0.2, None)


def slope_cases():
    for slope in SLOPES:
        for h, d in ((8, 16), (3, 5)):
            for kind in ("ties", "large"):
                yield ("slopes", TIES_GRAPH, 17, h, d, 5, kind, slope, None)


def dropout_cases():
    for h, d in ((4, 32), (3, 8)):
        yield ("dropout", HUB_GRAPH[32], 132, h, d, 40 + h, "unit", 0.2, DROP)


def other_cases():
    yield ("identity ids", HUB_GRAPH[32], None, 4, 16, 9, "unit", 0.2, None)
    yield ("zero edge rows", HUB_GRAPH[32], 132, 4, 16, 11, "zero", 0.2, None)
    for h, d in ((3, 8), (4, 16), (1, 64)):
        yield ("rectangular", RECT_GRAPH, 21, h, d, h, "unit", 0.2, None)
    for h, d in ((4, 16), (3, 5)):
        yield ("misaligned", BIND_GRAPH, 23, h, d, 3, "unit", 0.2, None)
    yield ("no dxe", WHOLE_ROWS_GRAPH, 23, 2, 32, 4, "unit", 0.2, None)


def all_cases():
    for gen in (parity_cases, slope_cases, dropout_cases, other_cases):
        yield from gen()


def sweep_case(seed):
    """the parameters of seed `seed` of the seeded sweep: (what, g', src, dst, h, d, slope, drop, need_dxe, dtype)"""
    import random
    rnd = random.Random(1000 + seed)
    n_src, n_dst = rnd.randint(20, 400), rnd.randint(20, 400)
    n_edges = rnd.randint(50, 3000)
    h, d = rnd.choice(FAST + [(3, 8), (1, 5), (5, 12), (2, 16)])
    chunk_size = rnd.choice((1, 3, 8, 32))
    slope = rnd.choice((0.2, 0.0, -0.1, 1.0, 0.01))
    p = rnd.choice((0.0, 0.0, 0.3, 0.6))
    permuted, need_dxe = rnd.random() < 0.7, rnd.random() < 0.7
    dtype = torch.float64 if rnd.random() < 0.25 else torch.float32
    hub = rnd.choice((None, min(n_edges // 2, 1200)))
    what = "seed %d: %dx%d E=%d (%d, %d) cs=%d slope=%g p=%g perm=%s dxe=%s %s hub=%s" % (
        seed, n_src, n_dst, n_edges, h, d, chunk_size, slope, p, permuted, need_dxe, dtype, hub)
    g0 = random_graph(n_src, n_dst, n_edges, seed=seed, chunk_size=chunk_size, zero_rows=0.15, hub=hub)
    g, src, dst = permute_edge_ids(g0, 77 + seed if permuted else None)
    drop = (p, 2 ** 40 + seed, seed) if p > 0 else None
    return what, g, src, dst, h, d, slope, drop, need_dxe, dtype


SWEEP_SEEDS = range(12)
CPG_SHAPES = (((1, 64), 0.0), ((4, 32), 0.3), ((8, 32), 0.0))      # one shape per row width, at cpg = 2


def cpg_inputs(src, dst, g, hd):
    return inputs(src, dst, g.n_src, g.n_dst, hd[0], hd[1], torch.float32, seed=20 + hd[0])


_GRAPHS = {}
_REFS = {}


def case_graph(make, perm_seed):
    """(g', src, dst) of a case, built once"""
    key = (make, perm_seed)
    if key not in _GRAPHS:
        _GRAPHS[key] = permute_edge_ids(make(), perm_seed)
    return _GRAPHS[key]


def case_inputs(case, dtype=torch.float64):
    _, make, perm_seed, h, d, seed, kind, _, _ = case
    g, src, dst = case_graph(make, perm_seed)
    return inputs(src, dst, g.n_src, g.n_dst, h, d, dtype, seed, kind)


def case_reference(case, inp=None, dtype=torch.float64):
    """the float64 reference of a case on its own inputs is computed once and shared (never modified)"""
    _, make, perm_seed, _, _, _, _, slope, drop = case
    g, src, dst = case_graph(make, perm_seed)
    p, seed, offset = drop or (0.0, 0, 0)
    if inp is None:
        key = (case[0], make, perm_seed) + tuple(case[3:])
        if key not in _REFS:
            _REFS[key] = reference(src, dst, g.n_src, *case_inputs(case), slope, p, seed, offset)
        return _REFS[key]
    return reference(src, dst, g.n_src, *inp, slope, p, seed, offset, dtype)
