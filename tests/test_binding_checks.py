"""GPU tier: the argument checks of the three Python-facing surfaces (graphop.*, graphop_cpp.*, torch.ops.graphop.*)
refuse the same defective calls with the same kind of message, for every op.  One well-formed call per op and surface
passes; every other call differs from it in one argument and raises before anything is launched.  Every spoiled
argument is at least as large in memory as the one it replaces, so a check that went missing would still read and write
inside the allocations."""
import pytest
import torch

from custom_op_benchmark_amd import _ext
from custom_op_benchmark_amd import graphop as ops

from util import random_graph

pytestmark = pytest.mark.gpu

N, H, D = 12, 2, 4
ROW = ("row", "indptr", "eid")
ROW_I = ROW + ("indices",)
BOTH_RC = ("row", "indptr_r", "eid_r", "indices_r", "col", "indptr_c", "eid_c", "indices_c")
BOTH_T = ROW_I + ("col", "indptr_t", "eid_t", "indices_t")
GAT_BWD = ("el", "er", "V", "o", "stats", "dO")
GATV2_BWD = ("xl", "xr", "att", "o", "stats", "dO")
# op: (its index arrays, its value operands, its trailing scalars)
OPS = {
    "maskedmm_csr_forward": (ROW_I, ("A", "B"), ()),
    "maskedmm_csr_backward": (BOTH_RC, ("A", "B", "dy"), ()),
    "node_mul_edge_forward": (ROW, ("A", "Be"), ()),
    "node_mul_edge_backward": (ROW, ("A", "Be", "dy"), ()),
    "sparse_softmax_forward": (ROW, ("xe",), ()),
    "sparse_softmax_backward": (ROW, ("y", "dy"), ()),
    "vector_spmm_forward": (ROW_I, ("edata", "x"), ()),
    "vector_spmm_backward": (BOTH_T, ("edata", "dyn", "x"), ()),
    "attention_forward": (ROW_I, ("Q", "K", "V"), ()),
    "attention_backward": (BOTH_RC, ("Q", "K", "V", "o", "stats", "dO"), ()),
    "gat_scores_forward": (ROW_I, ("el", "er"), ()),
    "gat_scores_backward": (BOTH_RC, ("el", "er", "dy"), ()),
    "gat_attention_forward": (ROW_I, ("el", "er", "V"), ()),
    "gat_attention_backward": (BOTH_RC, GAT_BWD, ()),
    "gat_attention_dropout_forward": (ROW_I, ("el", "er", "V"), (0.2, 0.5, 3, 1)),
    "gat_attention_dropout_backward": (BOTH_RC, GAT_BWD, (0.2, 0.5, 3, 1)),
    "edge_dropout_mask": (ROW_I, (), (H, 0.5, 3, 1)),
    "gatv2_scores_forward": (ROW_I, ("xl", "xr", "att"), ()),
    "gatv2_scores_backward": (BOTH_RC, ("xl", "xr", "att", "dy"), ()),
    "gatv2_attention_forward": (ROW_I, ("xl", "xr", "att"), ()),
    "gatv2_attention_backward": (BOTH_RC, GATV2_BWD, ()),
    "gatv2_attention_dropout_forward": (ROW_I, ("xl", "xr", "att"), (0.2, 0.5, 3, 1)),
    "gatv2_attention_dropout_backward": (BOTH_RC, GATV2_BWD, (0.2, 0.5, 3, 1)),
    "gat_edge_attention_forward": (ROW_I, ("el", "er", "ee", "V"), (0.2, 0.5, 3, 1)),
    "gat_edge_attention_backward": (BOTH_RC, ("el", "er", "ee", "V", "o", "stats", "dO"), (0.2, 0.5, 3, 1)),
}
# the operand's name in the signature (and in the messages) where the table above had to tell two shapes apart
SPELLED = {"Be": "B", "dyn": "dy", "xe": "x"}
GRADIENTS = ("dy", "dO")          # made contiguous by the op; the C++ messages spell them dy_ / dO_ where they say CUDA
# (op, operand): the operand must hold one entry per edge id
EDGE_ROWS = (("maskedmm_csr_backward", "dy"), ("node_mul_edge_backward", "dy"), ("sparse_softmax_forward", "xe"),
             ("sparse_softmax_backward", "y"), ("sparse_softmax_backward", "dy"), ("vector_spmm_forward", "edata"),
             ("vector_spmm_backward", "edata"))
# the float64 operand is the second value operand, named after the first in the message, except here
FLOAT64 = {"sparse_softmax_backward": ("y", "y and dy"), "vector_spmm_backward": ("x", "edata and x")}
# operand: (the dimension that gets one entry too many, what the message says), for every op that has the operand
WRONG_SHAPE = {"stats": (2, "stats"), "dO": (0, "dO must match"), "ee": (0, "ee must be (n_edges)"),
               "att": (1, "att must be")}


def _shape(name, e):
    return {"A": (N, H, D), "B": (N, H, D), "Be": (e, D), "x": (N, H, D), "dyn": (N, H, D), "Q": (N, H, D),
            "K": (N, H, D), "V": (N, H, D), "o": (N, H, D), "dO": (N, H, D), "xl": (N, H, D), "xr": (N, H, D),
            "el": (N, H), "er": (N, H), "att": (H, D), "stats": (N, H, 2),
            "dy": (e, H), "y": (e, H), "edata": (e, H), "ee": (e, H), "xe": (e, H)}[name]


def _cases(e):
    """-> [(op, label, operand to replace, how, substrings of the message)]"""
    out = []
    for op, (index, values, _) in OPS.items():
        spelled = [SPELLED.get(v, v) for v in values]
        plain = [v for v in values if op == "vector_spmm_backward" or v not in GRADIENTS]
        if plain:
            v = plain[0]
            out.append((op, "strided", v, "strided", (SPELLED.get(v, v) + " must be contiguous",)))
        bad = [n for n in index if n.startswith("eid")][-1]        # of the second orientation where there are two
        out.append((op, "int32", bad, "int32", ("expected scalar type Long but found", "(%s)" % bad)))
        if op in FLOAT64 or len(plain) > 1:
            v, pair = FLOAT64.get(op) or (plain[1], "%s and %s" % (spelled[0], SPELLED.get(plain[1], plain[1])))
            out.append((op, "float64", v, "float64", ("expected %s to have the same dtype" % pair,)))
        for v in values:
            if SPELLED.get(v, v) in GRADIENTS:
                out.append((op, "cpu " + v, v, "cpu", (SPELLED.get(v, v), " must be a CUDA tensor")))
            if v in WRONG_SHAPE and not (op == "attention_backward" and v == "dO"):
                out.append((op, "shape " + v, v, "grown", (op + ": ", WRONG_SHAPE[v][1])))
        if op == "attention_backward":
            out.append((op, "shape dO", "dO", "grown", ("attention_backward: o, dO must match Q",)))
        if op.endswith("scores_backward"):
            out.append((op, "shape dy", "dy", "grown", (op + ": dy must hold (n_edges, h)",)))
    for op, v in EDGE_ROWS:
        out.append((op, "short " + v, v, "short", ("%s must hold one entry per edge id: %d rows for %d edges"
                                                   % (SPELLED.get(v, v), e - 1, e),)))
    return out


def _spoil(t, how, name):
    if how == "strided":          # the same shape over rows twice as long
        wide = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
        bad = wide[..., :t.shape[-1]]
        assert not bad.is_contiguous()
        return bad
    if how == "int32":            # the same ids, in a buffer as large as the int64 one
        bad = torch.zeros(2 * t.numel(), dtype=torch.int32, device=t.device)[:t.numel()]
        bad.copy_(t)
        return bad
    if how == "float64":
        return t.double()
    if how == "cpu":
        return t.cpu()
    if how == "short":            # a contiguous prefix view of the full-length tensor
        bad = t[:t.size(0) - 1]
        assert bad.is_contiguous() and bad.data_ptr() == t.data_ptr()
        return bad
    assert how == "grown"
    dim = WRONG_SHAPE[name][0] if name in WRONG_SHAPE else 0
    shape = list(t.shape)
    shape[dim] += 1
    return torch.zeros(shape, dtype=t.dtype, device=t.device)


def test_every_surface_refuses_the_same_defects(dev):
    ext = _ext.load()
    assert ext is not None and ops.cpp_ext is ext, "graphop_cpp.so not built (run __graft_entry__.build())"
    g = random_graph(N, N, 40, seed=1, chunk_size=4).to(dev)
    e = g.n_edges
    gen = torch.Generator(device=dev).manual_seed(2)
    arrays = dict(zip(BOTH_RC, g.csr_args()))
    arrays.update(zip(BOTH_T, g.csr_args()))
    good = {n: torch.rand(_shape(n, e), device=dev, generator=gen) for n in
            sorted({v for _, values, _ in OPS.values() for v in values})}
    surfaces = (("graphop", lambda op: getattr(ops, op)), ("graphop_cpp", lambda op: getattr(ext, op)),
                ("torch.ops.graphop", lambda op: getattr(torch.ops.graphop, op)))
    assert set(OPS) == set(ops._SCHEMAS)

    def call(fn, op, replaced=None, bad=None):
        index, values, scalars = OPS[op]
        args = [arrays[n] for n in index] + [good[n] for n in values]
        if replaced is not None:
            args[(index + values).index(replaced)] = bad
        return fn(*args, *scalars)

    for op in OPS:                                                      # the control: nothing is refused
        for _, surface in surfaces:
            call(surface(op), op)
    torch.cuda.synchronize()
    cases = _cases(e)
    assert {(op, v) for op, label, v, how, _ in cases if how == "short"} == set(EDGE_ROWS)
    for op, label, replaced, how, substrings in cases:
        source = arrays[replaced] if replaced in arrays else good[replaced]
        bad = _spoil(source, how, replaced)
        for where, surface in surfaces:
            with pytest.raises(RuntimeError) as err:
                call(surface(op), op, replaced, bad)
            for s in substrings:
                assert s in str(err.value), (where, op, label, str(err.value))
    torch.cuda.synchronize()
