"""CPU statement of the fused dot-product attention step with edge-type embeddings (include/graphop_hip.h, DESIGN.md
4.5o): attention_edge_reference.reference_step on xe = R[etype], and dR = zeros_like(R).index_add(0, etype, dxe).  Also
the named input sets of the GPU tier (tests/test_attention_etype.py): a graph, the inputs of the edge-feature op's tier
(Q, dO ~ randn / sqrt(d); K, V ~ randn), R ~ randn, etype and n_types."""
import math

import torch

import attention_edge_reference as E

KEYS = ("o", "dQ", "dK", "dV", "dR")
PLAIN = ("o", "dQ", "dK", "dV")
HD = E.HD
DROP, NONE = E.DROP, E.NONE
TABLE_BYTES = 16384          # kAttnEtypeTableBytes: the fast row pass sums dR in at most this much LDS


def max_types(h, d):
    """kAttnEtypeMaxTypes of an (h, d): the largest table the fast row pass with dR takes"""
    return TABLE_BYTES // (4 * h * d)


def reference_step(src, dst, n_q, Q, K, V, R, etype, dO, p=0.0, seed=0, offset=0, head0=0, dtype=torch.float64):
    """-> dict(o, dQ, dK, dV, dR, dxe, stats) in `dtype`; dR in R's shape, dxe the (E, ...) gradient it is summed from"""
    t = etype.long()
    out = E.reference_step(src, dst, n_q, Q, K, V, R.to(dtype)[t], dO, p, seed, offset, head0, dtype)
    out["dR"] = torch.zeros(R.shape, dtype=dtype).index_add(0, t, out["dxe"])
    return out


def n_max(etype, n_types):
    """the largest edge count of one type"""
    return int(torch.bincount(etype.long().clamp(0, n_types - 1), minlength=n_types).max())


def tol(dtype, p=0.0, factor=1, key=None, n_max=0):
    """attention_edge_reference.tol; for dR -- a sum over all edges of a type, not over one row -- atol times
    max(1, sqrt(n_max / 2700)): an fp32 sum's rounding error grows with the square root of its length, and 2700 is the
    edge count at which the unscaled bound was checked"""
    t = E.tol(dtype, p, factor)
    if key == "dR" and dtype != torch.float64:
        t["atol"] *= max(1.0, math.sqrt(n_max / 2700.0))
    return t


def hub_row(g):
    return int(torch.bincount(g.src, minlength=g.n_src).argmax())


def make_types(g, n_types, seed):
    """(E,) int32 by edge id, uniform over the types with, where there are enough of them, the LAST type carried by no
    edge (its dR is exactly 0) and the one before it carried by every other edge of the hub row and by no other edge
    (its adds come from the several workgroups the hub row is split over)"""
    gen = torch.Generator().manual_seed(1000 + seed)
    free = n_types - (2 if n_types > 3 else 1 if n_types > 2 else 0)
    t = torch.randint(0, free, (g.n_edges,), generator=gen)
    if n_types > 3:
        hub = torch.nonzero(g.src == hub_row(g))[:, 0]
        t[hub[::2]] = n_types - 2
    return t.to(torch.int32)


def inputs(g, h, d, dtype, seed, n_types):
    """(Q, K, V, R, etype, dO) on the CPU; h == 1 gives 2-D operands"""
    Q, K, V, _, dO = E.inputs(g.n_src, g.n_dst, 0, h, d, dtype, seed)
    gen = torch.Generator().manual_seed(77 + seed)
    R = torch.randn(*((n_types, d) if h == 1 else (n_types, h, d)), generator=gen, dtype=torch.float64).to(dtype)
    return Q, K, V, R, make_types(g, n_types, seed), dO


# name -> (graph builder, graph seed or None, h, d, input seed, n_types); float32 all
INPUT_SETS = {"pair_%d_%d" % hd: (E.tier_graph, 3, hd[0], hd[1], hd[0] * 100 + hd[1], 5) for hd in HD}
INPUT_SETS.update({"types_%d" % n: (E.tier_graph, 3, 4, 16, 40 + n, n) for n in (1, 5, max_types(4, 16), max_types(4, 16) + 1)})
INPUT_SETS.update({
    "types_8_32_max": (E.tier_graph, 3, 8, 32, 832, max_types(8, 32)),
    "edge_ids": (E.tier_graph, 9, 4, 16, 6, 5),
    "cross": (E.tier_graph, 3, 4, 16, 21, 7),
    "need_dr": (E.tier_graph, 3, 4, 16, 8, 6),
    "clamp": (E.tier_graph, 3, 4, 16, 9, 4),
    "generic_3_5": (E.tier_graph, 3, 3, 5, 305, 5),
    "generic_4_16": (E.tier_graph, 3, 4, 16, 41, 5),
    "chunky": (E.chunky_graph, None, 4, 16, 2, 16),
    "head0": (E.tier_graph, 3, 4, 16, 31, 5),
    "autograd_8_32": (E.tier_graph, 3, 8, 32, 5, 9),
})


def input_set(name):
    """-> (graph, (Q, K, V, R, etype, dO), n_types) of a named set"""
    build, gseed, h, d, seed, n_types = INPUT_SETS[name]
    g = build() if gseed is None else build(gseed)
    return g, inputs(g, h, d, torch.float32, seed, n_types), n_types
