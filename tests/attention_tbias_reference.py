"""CPU statement of the fused dot-product attention step with an edge-type score bias (include/graphop_hip.h, DESIGN.md
4.5p): attention_bias_reference.attention_bias on b = B[clamped etype] in the dtype asked for (float64 by default; the
input-condition test evaluates it in float32), gradients from autograd, and dB[t] = db[etype == t].sum(0).  The row
statistics are those of the biased, undropped scores, (-1e9, 0) for rows without edges.  Also the named input sets of
the GPU tier (tests/test_attention_tbias.py): the graph recipe and the inputs of attention_etype_reference (Q, dO ~
randn / sqrt(d); K, V ~ randn), B ~ randn, etype and n_types."""
import math

import torch

import attention_bias_reference as AB
import attention_dropout_reference as A
import attention_edge_reference as E
import attention_etype_reference as ET

KEYS = ("o", "dQ", "dK", "dV", "dB")
PLAIN = ("o", "dQ", "dK", "dV")
HD = E.HD
DROP, NONE = E.DROP, E.NONE
TABLE_BYTES = 16384          # kAttnTbiasTableBytes: the fast row pass sums dB in at most this much LDS
# the bounds of the per-edge bias op's tier (tests/test_attention_bias.py: TOL of tests/test_fused_attention.py)
TOL32 = dict(rtol=1e-4, atol=1e-5)
TOL64 = dict(rtol=1e-10, atol=1e-12)
hub_row = ET.hub_row
make_types = ET.make_types
error_ratio = E.error_ratio


def max_types(h):
    """the largest table the fast row pass with dB takes: n_types * h words in kAttnTbiasTableBytes"""
    return TABLE_BYTES // (4 * h)


def clamped(etype, n_types):
    """min((unsigned) etype, n_types - 1) as the kernels take it: negative values are large unsigned ones"""
    t = etype.long()
    return torch.where((t < 0) | (t > n_types - 1), torch.full_like(t, n_types - 1), t)


def gathered(B, etype):
    """b = B[clamped etype]: (E) for 1-D B, else (E, h)"""
    return B[clamped(etype, B.size(0))]


def reference_step(src, dst, n_q, Q, K, V, B, etype, dO, p=0.0, seed=0, offset=0, head0=0, dtype=torch.float64):
    """-> dict(o, dQ, dK, dV, dB, db, stats) in `dtype`; dB in B's shape, db the (E[, h]) gradient it is summed from"""
    t = clamped(etype, B.size(0))
    q, k, v = (x.to(dtype).clone().requires_grad_(True) for x in (Q, K, V))
    b = B.to(dtype)[t].clone().requires_grad_(True)
    o = AB.attention_bias(src, dst, n_q, q, k, v, b, p, seed, offset, head0)
    o.backward(dO.to(dtype))
    m, l = A.softmax_stats(src, n_q, AB.biased_scores(src, dst, q.detach(), k.detach(), b.detach()))
    stats = torch.stack([m, torch.where(l > 0, 1 / l, torch.zeros_like(l))], -1)
    dB = torch.zeros(B.shape, dtype=dtype).index_add(0, t, b.grad)
    return dict(o=o.detach(), dQ=q.grad, dK=k.grad, dV=v.grad, dB=dB, db=b.grad, stats=stats)


def n_max(etype, n_types):
    """the largest edge count of one type"""
    return int(torch.bincount(clamped(etype, n_types), minlength=n_types).max())


def tol(dtype, p=0.0, factor=1, key=None, n_max=0):
    """The per-edge bias op's bounds: fp32 rtol 1e-4 / atol 1e-5 / (1 - p) -- every term of every sum is scaled by the
    multiplier -- or fp64 1e-10 / 1e-12; factor 2 for two fp32 results compared with each other.  dB[t] is a sum of
    n_max values db[e] at the most, each held to db's bound: its atol is db's times sqrt(n_max), the growth of a sum of
    independent errors (attention_etype_reference.tol scales dR's the same way)."""
    t = dict(TOL64) if dtype == torch.float64 else dict(rtol=factor * TOL32["rtol"], atol=factor * TOL32["atol"] / (1 - p))
    if key == "dB":
        t["atol"] *= math.sqrt(max(1, n_max))
    return t


def inputs(g, h, d, dtype, seed, n_types):
    """(Q, K, V, B, etype, dO) on the CPU; h == 1 gives 2-D operands and a 1-D B"""
    Q, K, V, _, dO = E.inputs(g.n_src, g.n_dst, 0, h, d, dtype, seed)
    gen = torch.Generator().manual_seed(177 + seed)
    B = torch.randn(*((n_types,) if h == 1 else (n_types, h)), generator=gen, dtype=torch.float64).to(dtype)
    return Q, K, V, B, make_types(g, n_types, seed), dO


# name -> (graph builder, graph seed or None, h, d, input seed, n_types); float32 all
INPUT_SETS = {"pair_%d_%d" % hd: (E.tier_graph, 3, hd[0], hd[1], hd[0] * 100 + hd[1], 5) for hd in HD}
INPUT_SETS.update({"types_%d" % n: (E.tier_graph, 3, 8, 8, 60 + n % 7, n) for n in (1, max_types(8), max_types(8) + 1)})
INPUT_SETS.update({
    "edge_ids": (E.tier_graph, 9, 4, 16, 6, 5),
    "partial": (E.tier_graph, 3, 4, 16, 8, 6),
    "need_db": (E.tier_graph, 3, 4, 16, 8, 6),
    "clamp": (E.tier_graph, 3, 4, 16, 9, 4),
    "weights": (E.tier_graph, 3, 4, 16, 21, 7),
    "generic_3_5": (E.tier_graph, 3, 3, 5, 305, 5),
    "generic_4_16": (E.tier_graph, 3, 4, 16, 41, 5),
    "head0": (E.tier_graph, 3, 4, 16, 31, 5),
    "autograd_8_32": (E.tier_graph, 3, 8, 32, 5, 9),
})


def input_set(name):
    """-> (graph, (Q, K, V, B, etype, dO), n_types) of a named set"""
    build, gseed, h, d, seed, n_types = INPUT_SETS[name]
    g = build() if gseed is None else build(gseed)
    return g, inputs(g, h, d, torch.float32, seed, n_types), n_types
