"""CPU tier of the attention weights of the fused GAT and GATv2 layers (graphop_gat_attention_weights,
graphop_gatv2_attention_weights, functions.FusedGATAttentionWeights / FusedGATv2AttentionWeights): the
formulas the ops and the classes implement equal autograd through the float64 references, the library and the bindings
expose the ops and validate their arguments before anything touches a device, the gfx950 code object holds exactly the
k_gatw_* / k_gv2w_* instantiations the ops launch and keeps every one out of scratch, and the inputs the GPU tier uses
are ones on which torch's own fp32 arithmetic stays within half of that tier's bounds."""
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch

import gat_edge_reference as GE
import gatv2_edge_reference as G2
import gat_weights_reference as W
from fused_gatv2_reference import K32, datt_ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gat_attention_weights", "gatv2_attention_weights")
F64 = torch.float64
CLOSE = dict(rtol=1e-12, atol=1e-12)


def _small_graph(gen, n_l=23, n_r=17):
    """rectangular, rows without edges (every fifth), parallel edges (the diagonal is added twice): the graph of
    tests/test_attention_weights_host.py, restated"""
    src = torch.randint(0, n_l, (160,), generator=gen)
    src = src[src % 5 != 0]
    dst = torch.randint(0, n_r, (src.numel(),), generator=gen)
    diag = torch.arange(1, n_r)
    diag = diag[diag % 5 != 0]
    return torch.cat([src, diag, diag]), torch.cat([dst, diag, diag])


def _case(kind, h, seed=3, n_l=23, n_r=17, d=5):
    gen = torch.Generator().manual_seed(seed)
    src, dst = _small_graph(gen, n_l, n_r)
    mod = GE if kind == W.GAT else G2
    first, second, edge, last, dO = mod.inputs(src, dst, n_l, n_r, h, d, F64, seed)
    ga = W.ga_inputs(src.numel(), h, seed, F64)
    assert n_l != n_r and (torch.bincount(src, minlength=n_l) == 0).any()
    assert torch.unique(torch.stack([src, dst], 1), dim=0).size(0) < src.numel()          # parallel edges
    return src, dst, n_l, n_r, (first, second, edge, last), dO, ga


def _gat_layer_weights(src, dst, n_l, el, er, ee, slope):
    """a (E, h) out of gat_edge_reference.gat_edge_layer itself: every edge gets a neighbour row of its own, whose V row
    is its unit vector, so that o[src[e], :, e] = a_e; autograd-able in el, er and ee"""
    E = src.numel()
    own = torch.arange(E)
    V = torch.eye(E, dtype=F64)
    if el.dim() == 2:
        V = V[:, None, :].expand(E, el.size(1), E)
    o = GE.gat_edge_layer(src, own, n_l, el, er[dst], ee, V, slope)
    return o[src, own][:, None] if el.dim() == 1 else o[src, :, own]


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("h", [1, 3])
@pytest.mark.parametrize("kind", [W.GAT, W.GATV2])
def test_restated_weights_and_gradients_match_autograd(kind, h, edge):
    """a = exp(min(s - m, 0)) * linv from the statistics, row sums of 1, the ga path of the three differentiable forms as
    the classes compute it, the sum of both paths with dO too, and a independent of p, against autograd through the
    float64 references (gat_edge_layer, layer_head: an absent edge operand is a zero one there) at 1e-12"""
    slope = 0.2
    src, dst, n_l, n_r, ops, dO, ga = _case(kind, h)
    ops = W.with_edge(ops, edge)
    zero_edge = torch.zeros_like(_case(kind, h)[4][2])
    full = ops if edge else (ops[0], ops[1], zero_edge, ops[3])
    only_a = W.step(kind, src, dst, n_l, ops, None, ga, slope)
    a2 = only_a["a"].reshape(src.numel(), -1)
    # the op's formula on the reference's own statistics
    torch.testing.assert_close(W.restated_weights(src, only_a["s"], only_a["stats"]), a2, **CLOSE)
    rows = torch.zeros(n_l, a2.size(1), dtype=F64).index_add(0, src, a2)
    has = torch.bincount(src, minlength=n_l) > 0
    torch.testing.assert_close(rows[has], torch.ones_like(rows[has]), **CLOSE)
    assert not only_a["stats"][~has][..., 1].any()
    only_o = W.step(kind, src, dst, n_l, ops, dO, None, slope, 0.6, 99, 2)
    both = W.step(kind, src, dst, n_l, ops, dO, ga, slope, 0.6, 99, 2)
    assert torch.equal(both["a"], only_a["a"])          # the undropped weights, whatever p
    names = [n for n, t in zip(W.OPERANDS[kind], ops) if t is not None]
    # against the reference modules
    if kind == W.GAT:
        leaf = [t.clone().requires_grad_(True) for t in full[:3]]
        a_ref = _gat_layer_weights(src, dst, n_l, *leaf, slope)
        torch.testing.assert_close(a_ref.detach(), a2, **CLOSE)
        (a_ref * ga.reshape(a_ref.shape)).sum().backward()
        for n, t in zip(("el", "er", "ee"), leaf):
            if n in names:
                torch.testing.assert_close(only_a["d" + n], t.grad, **CLOSE, msg=lambda m: n + ": " + m)
        assert not only_a["dV"].any()          # a does not depend on V
        want = GE.reference(src, dst, n_l, *full, dO, slope, 0.6, 99, 2)
        ref = dict(zip(("o", "del", "der", "dee", "dV"), want))
    else:
        want = G2.reference(src, dst, n_l, full[0], full[1], full[2], full[3], dO, slope, 0.6, 99, 2)
        ref = dict(zip(("o", "dxl", "dxr", "dxe", "datt"), want[:5]))
        torch.testing.assert_close(only_a["stats"], want[6], **CLOSE)
        for k in range(h):
            pick = (lambda t: t) if h == 1 else (lambda t: t[:, k])
            _, s_k = G2.layer_head(src, dst, n_l, pick(full[0]), pick(full[1]), pick(full[2]),
                                   full[3] if h == 1 else full[3][k], slope)
            torch.testing.assert_close(only_a["s"][:, k], s_k, **CLOSE)
    torch.testing.assert_close(only_o["o"], ref["o"], **CLOSE)
    for n in names:
        torch.testing.assert_close(only_o["d" + n], ref["d" + n], **CLOSE, msg=lambda m: n + ": " + m)
        torch.testing.assert_close(both["d" + n], only_o["d" + n] + only_a["d" + n], **CLOSE, msg=lambda m: n + ": " + m)
    # the ga path as the classes compute it
    if kind == W.GATV2 and edge:
        return          # the class marks a non-differentiable there
    got = W.restated_ga(kind, src, dst, n_l, n_r, ops, a2, ga.reshape(a2.shape), slope)
    for key, name in (("del_", "del"), ("der", "der"), ("dee", "dee"), ("dxl", "dxl"), ("dxr", "dxr"), ("datt", "datt")):
        if key in got:
            torch.testing.assert_close(got[key].reshape(only_a[name].shape), only_a[name], **CLOSE,
                                       msg=lambda m: name + ": " + m)


def _slopes_of(name):
    return W.SLOPES if "ties" in name else (0.2,)


@pytest.mark.parametrize("name", sorted(W.INPUT_SETS))
def test_input_condition(name):
    """Torch's own float32 evaluation of the reference against the float64 one stays within 0.5 of the GPU tier's bounds
    (TOL_A for a; TOL32 / gatv2_edge_reference.tol for o and the gradients, the ga term included where a is
    differentiable; datt against K32 S) on every input set, edge form and slope that tier uses (tests/test_gat_weights.py
    takes its graphs and operands from gat_weights_reference.INPUT_SETS only, or from the same generators), and |s| < 9: the bounds
    leave a kernel that sums in another order the other half."""
    kind, g, src, dst, ops, dO, ga, h, d = W.input_set(name)
    tol = GE.TOL32 if kind == W.GAT else G2.tol(torch.float32)
    for slope in _slopes_of(name):
        for edge in (False, True):
            o = W.with_edge(ops, edge)
            gg = None if (kind == W.GATV2 and edge) else ga
            want = W.step(kind, src, dst, g.n_src, o, dO, gg, slope)
            got = W.step(kind, src, dst, g.n_src, o, dO, gg, slope, dtype=torch.float32)
            ratios = {"a": W.error_ratio(got["a"], want["a"], **W.TOL_A)}
            for k in ["o"] + ["d" + n for n, t in zip(W.OPERANDS[kind], o) if t is not None]:
                if k == "datt":
                    ratios[k] = datt_ratio(got[k], want[k], want["S"]) / K32
                else:
                    ratios[k] = W.error_ratio(got[k], want[k], **tol)
            print(name, slope, edge, {k: round(v, 4) for k, v in ratios.items()})
            assert max(ratios.values()) <= 0.5, (name, slope, edge, ratios)
            assert float(want["s"].abs().max()) < 9, (name, slope, edge)


def _doc_args(fn):
    doc = fn.__doc__.splitlines()[0]
    return [a.split(":")[0] + (a[a.index(" = "):] if " = " in a else "")
            for a in doc[doc.index("(") + 1:doc.rindex(") -> ")].split(", ")]


def test_symbols_resolve_in_the_library_and_the_extension():
    from custom_op_benchmark_amd import _ext, _lib, functions, graphop as ops
    l = ctypes.CDLL(_lib.LIB_PATH)
    ext = _ext.load()
    assert ext is not None, "graphop_cpp.so not built (run __graft_entry__.build())"
    assert _lib.ABI_VERSION == 8 and _lib.lib().graphop_abi_version() == 8        # additive: the ABI number stays
    for name in NAMES:
        assert hasattr(l, "graphop_" + name) and "graphop_" + name in _lib.EXPORTED_SYMBOLS
        assert callable(getattr(ext, name)) and callable(getattr(ops, name))
        assert name in ops.EXTRA_OPS and name not in ops._SCHEMAS and not hasattr(torch.ops.graphop, name)
        assert name not in ops.__all__
    assert len(ops.__all__) == 8
    want = {"gat_attention_weights": ["row", "indptr", "eid", "indices", "el", "er", "stats", "ee = None",
                                      "negative_slope = 0.2"],
            "gatv2_attention_weights": ["row", "indptr", "eid", "indices", "xl", "xr", "att", "stats", "xe = None",
                                        "negative_slope = 0.2"]}
    for name in NAMES:
        assert _doc_args(getattr(ext, name)) == want[name]
        sig = inspect.signature(getattr(ops, name))
        assert list(sig.parameters) == [a.split(" = ")[0] for a in want[name]]
        assert sig.parameters[want[name][-2].split(" = ")[0]].default is None
        assert sig.parameters["negative_slope"].default == 0.2
    for cls in (functions.FusedGATAttentionWeights, functions.FusedGATv2AttentionWeights):
        assert issubclass(cls, torch.autograd.Function)
    assert callable(functions.fused_gat_attention_weights_step) and callable(functions.fused_gatv2_attention_weights_step)
    assert "non-differentiable" in functions.FusedGATv2AttentionWeights.__doc__
    assert "(E, h, d)" in functions.FusedGATv2AttentionWeights.__doc__


def _call(l, v2, dtype, C, E_, n_l, n_r, h, d=8, stats=None, a=None, first=None, plan=None, csr=None):
    """csr: one dummy pointer for all four index arrays; plan: a host-side stand-in (by reference)"""
    n = ctypes.c_void_p(0)
    pl = ctypes.byref(plan) if plan is not None else n
    if v2:
        return l.graphop_gatv2_attention_weights(dtype, *([csr or n] * 4), first or n, n, n, n, stats or n, a or n, C, E_,
                                                 n_l, n_r, h, d, 0.2, pl, n)
    return l.graphop_gat_attention_weights(dtype, *([csr or n] * 4), first or n, n, n, stats or n, a or n, C, E_, n_l, n_r,
                                           h, 0.2, pl, n)


def _plan(arrays, n_chunks, n_edges, max_row, max_index):
    """a stand-in plan of the call's own index arrays (test_attention_heads_host.py's): the facts Csr::check_bounds
    reads, no device array behind it"""
    from test_attention_heads_host import _plan_struct
    plan = _plan_struct()()
    plan.info.n_chunks, plan.info.n_edges, plan.info.max_row, plan.info.max_index = n_chunks, n_edges, max_row, max_index
    plan.row = plan.indptr = plan.eid = plan.indices = arrays
    return plan


@pytest.mark.parametrize("v2", [False, True])
def test_a_matching_plan_must_bound_the_ids(v2):
    """The third check of the stated order: a plan of the call's own arrays whose largest row id or neighbour id lies
    outside the operands is an error (not a fall-back to the generic kernel), after the NULL checks of stats / a and
    before anything else is looked at; n_l bounds the row ids and n_r the neighbour ids, not the other way round"""
    from custom_op_benchmark_amd import _lib
    l = _lib.lib()
    some = ctypes.c_void_p(256)
    err = l.graphop_last_error
    fn = NAMES[v2].encode()
    first = b"xl / stats" if v2 else b"el / stats"
    second = b"xr" if v2 else b"er"
    C, E_, n_l, n_r = 4, 10, 7, 5
    rows = _plan(256, C, E_, n_l, n_r - 1)          # a row id one past el / stats
    assert _call(l, v2, 0, C, E_, n_l, n_r, 2, 8, some, some, plan=rows, csr=some) == 1
    assert fn + b": row id 7 but " + first + b" has only 7 rows" in err()
    idx = _plan(256, C, E_, n_l - 1, n_r)          # a neighbour id one past er
    assert _call(l, v2, 1, C, E_, n_l, n_r, 2, 8, some, some, plan=idx, csr=some) == 1
    assert fn + b": neighbour id 5 but " + second + b" has only 5 rows" in err()
    # row ids up to n_l - 1 > n_r - 1 are fine: the next complaint is the first operand, which the call left NULL
    ok = _plan(256, C, E_, n_l - 1, n_r - 1)
    assert _call(l, v2, 0, C, E_, n_l, n_r, 2, 8, some, some, plan=ok, csr=some) == 1
    assert fn + (b": xl is NULL" if v2 else b": el is NULL") in err()
    # the NULL checks of stats / a come first; a plan of other arrays is no plan of this call
    assert _call(l, v2, 0, C, E_, n_l, n_r, 2, 8, None, some, plan=rows, csr=some) == 1 and b"stats is NULL" in err()
    other = _plan(512, C, E_, n_l, n_r)
    assert _call(l, v2, 0, C, E_, n_l, n_r, 2, 8, some, some, plan=other, csr=some) == 1 and b" is NULL" in err()
    # an empty problem with such a plan is still refused: the bounds are checked before the early return
    assert _call(l, v2, 0, C, E_, 0, n_r, 2, 8, plan=_plan(256, C, E_, 0, 0), csr=some) == 1 and b"row id 0" in err()


@pytest.mark.parametrize("v2", [False, True])
def test_argument_validation_without_gpu(v2):
    """error code 1 (GRAPHOP_ERR_ARG) and the text, through ctypes with dummy pointers, in the order the header states:
    dtype and sizes (gat_check), then NULL stats / a, and only then the index arrays and the operands; empty problems
    return 0 and dereference nothing"""
    from custom_op_benchmark_amd import _lib
    l = _lib.lib()
    some = ctypes.c_void_p(256)
    err = l.graphop_last_error
    fn = NAMES[v2].encode()
    assert _call(l, v2, 7, 4, 10, 5, 5, 2, 8, some, some) == 1 and fn + b": dtype must be GRAPHOP_F32 or GRAPHOP_F64" in err()
    assert _call(l, v2, 2, 4, 10, 5, 5, 2) == 1 and fn + b": dtype must be" in err()          # before the NULL checks
    sizes = [(-1, 10, 5, 5, 2, 8), (4, -10, 5, 5, 2, 8), (4, 10, -5, 5, 2, 8), (4, 10, 5, -5, 2, 8), (4, 10, 5, 5, 0, 8)]
    if v2:
        sizes += [(4, 10, 5, 5, 2, 0), (4, 10, 5, 5, 2, -8)]
    for s in sizes:
        assert _call(l, v2, 0, *s) == 1 and fn + b": negative size" in err(), s          # before the NULL checks
    assert (b" d=" in err()) == v2          # the message of an op without a feature width has no d field
    for dtype in (0, 1):
        assert _call(l, v2, dtype, 4, 10, 5, 5, 2, 8, None, some) == 1 and fn + b": stats is NULL" in err()
        assert _call(l, v2, dtype, 4, 10, 5, 5, 2, 8, None, None) == 1 and fn + b": stats is NULL" in err()
        assert _call(l, v2, dtype, 4, 10, 5, 5, 2, 8, some, None) == 1 and fn + b": a is NULL" in err()
        # stats and a given: the index arrays come next, then the operands
        assert _call(l, v2, dtype, 4, 10, 5, 5, 2, 8, some, some) == 1 and fn + b": row is NULL" in err()
    # empty problems are no-ops that never dereference anything
    assert _call(l, v2, 0, 0, 0, 0, 0, 1) == 0
    assert _call(l, v2, 1, 0, 10, 5, 5, 2) == 0          # no chunks
    assert _call(l, v2, 0, 4, 0, 5, 5, 2) == 0           # no edges
    assert _call(l, v2, 0, 4, 10, 0, 5, 2) == 0          # no rows
    assert _call(l, v2, 1, 4, 10, 5, 0, 2) == 0          # no neighbour rows


def test_binding_refusals_without_gpu():
    """the index and value tensors first, then the operands in the words of the ops that already take them, stats and the
    edge operand"""
    from custom_op_benchmark_amd import graphop as ops
    i = torch.zeros(2, dtype=torch.int64)
    el, st = torch.zeros(2, 4), torch.zeros(2, 4, 2)
    xl, att = torch.zeros(2, 4, 8), torch.zeros(4, 8)
    for mod in (ops, ops.cpp_ext):
        with pytest.raises(RuntimeError, match="row must be a CUDA tensor"):
            mod.gat_attention_weights(i, i, i, i, el, el, st)
        with pytest.raises(RuntimeError, match="row must be a CUDA tensor"):
            mod.gatv2_attention_weights(i, i, i, i, xl, xl, att, st, xe=torch.zeros(2, 4, 8))
    fn = "gat_attention_weights"
    with pytest.raises(RuntimeError, match=r"gat_attention_weights: el \(n_src\[, h\]\) and er \(n_dst\[, h\]\) must have the same h"):
        ops._gat_heads(el, torch.zeros(2, 3), fn)
    for bad in (torch.zeros(2, 4, 3), torch.zeros(3, 4, 2), torch.zeros(2, 1, 2), torch.zeros(2, 8), torch.zeros(16)):
        with pytest.raises(RuntimeError, match=r"gat_attention_weights: stats must be \(n_src, h, 2\)"):
            ops._gat_weights_stats(fn, el, "el", bad, 4)
    with pytest.raises(RuntimeError, match=r"stats must be \(n_src, h, 2\)"):
        ops._gat_weights_stats(fn, el[:, 0], "el", st, 1)          # 1-D el is one head
    with pytest.raises(RuntimeError, match="expected el and stats to have the same dtype"):
        ops._gat_weights_stats(fn, el, "el", st.double(), 4)
    with pytest.raises(RuntimeError, match="expected xl and stats to have the same dtype"):
        ops._gat_weights_stats("gatv2_attention_weights", xl, "xl", st.double(), 4)
    assert ops._gat_weights_stats(fn, el, "el", st, 4) is None
    assert ops._gat_weights_stats(fn, el[:, 0], "el", st[:, :1], 1) is None
    # the edge operand is checked by the helpers of the ops that already take it, as an input first (the shape and
    # dtype wording of those helpers is exercised on the device, tests/test_gat_weights.py)
    with pytest.raises(RuntimeError, match="ee must be a CUDA tensor"):
        ops._gat_edge_term(el, torch.zeros(2, 4), 2, 4, fn)
    fn = "gatv2_attention_weights"
    with pytest.raises(RuntimeError, match="xe must be a CUDA tensor"):
        ops._gatv2_edge_rows(xl, torch.zeros(2, 4, 8), 2, 4, 8, fn)
    with pytest.raises(RuntimeError, match=r"gatv2_attention_weights: att must be"):
        ops._gatv2_shapes(xl, xl, torch.zeros(4, 4), fn)


def test_weights_kernels_census():
    """The exact instantiation sets of the k_gatw_* / k_gv2w_* kernels: 34, none with scratch or a spilled VGPR, under
    names that stay clear of the patterns that pin the kernels of the older ops."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources()
    mine = {n: r for n, r in res.items() if "k_gatw_" in n or "k_gv2w_" in n}
    fam = {}
    for n, r in mine.items():
        assert not r["spill_vgpr"] and not r["scratch"], (n, r)
        m = re.search(r"graphop::(k_g\w+)<(.*)>\(", n)
        assert m, n
        fam.setdefault(m.group(1), {})[m.group(2)] = r
    ty, tf = ("float", "double"), ("false", "true")
    want = {
        "k_gatw_f32": {"%d, %s" % (h, b) for h in W.FAST_H for b in tf},
        "k_gatw_generic": {"%s, %s" % (t, b) for t in ty for b in tf},
        "k_gv2w_f32": {"%d, %d, %s" % (h, d, b) for h, d in W.FAST_HD for b in tf},
        "k_gv2w_generic": {"%s, %s" % (t, b) for t in ty for b in tf},
    }
    assert set(fam) == set(want), sorted(set(fam) ^ set(want))
    for k in want:
        assert set(fam[k]) == want[k], (k, sorted(set(fam[k]) ^ want[k]))
    assert sum(len(v) for v in fam.values()) == len(mine) == 34
    pinned = r"k_gat_attn_|k_gat_edge_attn_|k_gatv2_|k_gv2attn_|k_gv2drop_|k_gv2e(dge|drop)_|k_attn_weights_"
    assert not [n for n in mine if re.search(pinned, n)]
    for k in ("k_gatw_f32", "k_gv2w_f32"):
        print("%s VGPRs: %d..%d" % (k, min(r["vgpr"] for r in fam[k].values()), max(r["vgpr"] for r in fam[k].values())))
    print("kernels that spill SGPRs:", {n: r["spill_sgpr"] for n, r in mine.items() if r["spill_sgpr"]})
