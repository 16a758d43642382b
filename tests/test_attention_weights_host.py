"""CPU tier of the attention weights of the fused dot-product attention ops (graphop_attention_weights,
functions.FusedAttentionWeights): the formulas the op and the class implement equal autograd through the
float64 reference, the library and the bindings expose the op and validate its arguments before anything touches a
device, the gfx950 code object holds exactly the k_attn_weights_* instantiations the op launches and keeps every one out
of scratch, and the inputs the GPU tier uses are ones on which torch's own fp32 arithmetic stays within half of that
tier's bounds."""
import ctypes
import os
import re
import sys

import pytest
import torch

import attention_edge_reference as E
import attention_weights_reference as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "attention_weights"


def _small_graph(gen, n_q=23, n_k=17):
    """rectangular, rows without edges (every fifth), parallel edges (the diagonal is added twice): the graph of
    tests/test_attention_edge_host.py, restated"""
    src = torch.randint(0, n_q, (160,), generator=gen)
    src = src[src % 5 != 0]
    dst = torch.randint(0, n_k, (src.numel(),), generator=gen)
    diag = torch.arange(1, n_k)
    diag = diag[diag % 5 != 0]
    return torch.cat([src, diag, diag]), torch.cat([dst, diag, diag])


def _case(h, seed=3, n_q=23, n_k=17, d=5):
    gen = torch.Generator().manual_seed(seed)
    src, dst = _small_graph(gen, n_q, n_k)
    Q, K, V, xe, dO = E.inputs(n_q, n_k, src.numel(), h, d, torch.float64, seed)
    shape = (src.numel(),) if h == 1 else (src.numel(), h)
    b, ga = (torch.randn(*shape, generator=gen, dtype=torch.float64) for _ in range(2))
    assert n_q != n_k and (torch.bincount(src, minlength=n_q) == 0).any()
    assert torch.unique(torch.stack([src, dst], 1), dim=0).size(0) < src.numel()          # parallel edges
    return src, dst, n_q, n_k, Q, K, V, xe, dO, b, ga


@pytest.mark.parametrize("mode", W.MODES)
@pytest.mark.parametrize("h", [1, 3])
def test_restated_weights_and_gradients_match_autograd(h, mode):
    """a = exp(min(s - m, 0)) * linv from the statistics, and (plain, bias) the ga path ds' = a (ga - sum a ga), dQ' = sum
    ds' K_j, dK' = sum ds' Q_i, db' = ds', against autograd through the reference, in float64 at 1e-12; with dO too the
    gradients are the sum of the fused backward's and the ga path's"""
    src, dst, n_q, n_k, Q, K, V, xe, dO, b, ga = _case(h)
    b, xe = W.mode_operands(mode, b, xe)
    want = W.reference_step(src, dst, n_q, Q, K, V, None, ga, b, xe)
    s = W.mode_scores(src, dst, Q, K, b, xe)
    m, linv = want["stats"][..., 0], want["stats"][..., 1]
    a = torch.exp(torch.clamp(s - m[src], max=0.0)) * linv[src]
    close = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(W.edge_shape(a, Q), want["a"], **close)
    rows = torch.zeros(n_q, a.size(1), dtype=torch.float64).index_add(0, src, a)
    has = torch.bincount(src, minlength=n_q) > 0
    torch.testing.assert_close(rows[has], torch.ones_like(rows[has]), **close)
    assert not want["dV"].any()          # a does not depend on V
    if mode == "edge":
        return          # the class marks a non-differentiable there
    ds, dQ, dK = W.restated_ga(src, dst, n_q, n_k, Q, K, a, W._two(ga))
    for name, got in (("dQ", dQ), ("dK", dK)) + ((("db", ds),) if mode == "bias" else ()):
        torch.testing.assert_close(got.reshape(want[name].shape), want[name], **close, msg=lambda t: name + ": " + t)
    both = W.reference_step(src, dst, n_q, Q, K, V, dO, ga, b, xe, 0.6, 99, 2)
    only_o = W.reference_step(src, dst, n_q, Q, K, V, dO, None, b, xe, 0.6, 99, 2)
    for name in ("dQ", "dK", "dV") + (("db",) if mode == "bias" else ()):
        torch.testing.assert_close(both[name], only_o[name] + want[name], **close, msg=lambda t: name + ": " + t)
    assert torch.equal(both["a"], want["a"])          # the undropped weights, whatever p


@pytest.mark.parametrize("name", sorted(W.INPUT_SETS))
def test_input_condition(name):
    """Torch's own float32 evaluation of the reference against the float64 one stays within 0.5 of the GPU tier's bounds
    (TOL_A for a, attention_edge_reference.tol for the rest, the ga term included) on every input set and mode that
    tier uses, and |s| < 9: the bounds leave a kernel that sums in another order the other half."""
    g, inp, (b, ga) = W.input_set(name)
    Q, K, V, xe, dO = inp
    src, dst = g.src, g.dst
    for mode in W.MODES:
        bb, x = W.mode_operands(mode, b, xe)
        gg = None if mode == "edge" else ga
        want = W.reference_step(src, dst, g.n_src, Q, K, V, dO, gg, bb, x)
        got = W.reference_step(src, dst, g.n_src, Q, K, V, dO, gg, bb, x, dtype=torch.float32)
        ratios = {"a": E.error_ratio(got["a"], want["a"], **W.TOL_A)}
        keys = ("o", "dQ", "dK", "dV") + (("db",) if mode == "bias" else ()) + (("dxe",) if mode == "edge" else ())
        ratios.update({k: E.error_ratio(got[k], want[k], **E.tol(torch.float32)) for k in keys})
        print(name, mode, {k: round(v, 4) for k, v in ratios.items()})
        assert max(ratios.values()) <= 0.5, (name, mode, ratios)
        assert float(W.mode_scores(src, dst, Q, K, bb, x).abs().max()) < 9, (name, mode)


def test_symbols_resolve_in_the_library_and_the_extension():
    import inspect
    from custom_op_benchmark_amd import _ext, _lib, functions, graphop as ops
    l = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(l, "graphop_" + NAME) and "graphop_" + NAME in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 8 and _lib.lib().graphop_abi_version() == 8        # additive: the ABI number stays
    ext = _ext.load()
    assert ext is not None, "graphop_cpp.so not built (run __graft_entry__.build())"
    assert callable(getattr(ext, NAME)) and callable(getattr(ops, NAME))
    assert NAME in ops.EXTRA_OPS and NAME not in ops._SCHEMAS and not hasattr(torch.ops.graphop, NAME)
    assert len(ops.__all__) == 8 and NAME not in ops.__all__
    doc = getattr(ext, NAME).__doc__.splitlines()[0]
    args = [a.split(":")[0] + (a[a.index(" = "):] if " = " in a else "")
            for a in doc[doc.index("(") + 1:doc.rindex(") -> ")].split(", ")]
    assert args == ["row", "indptr", "eid", "indices", "Q", "K", "stats", "b = None", "xe = None"], doc
    sig = inspect.signature(ops.attention_weights)
    assert list(sig.parameters) == ["row", "indptr", "eid", "indices", "Q", "K", "stats", "b", "xe"]
    assert sig.parameters["b"].default is None and sig.parameters["xe"].default is None
    assert issubclass(functions.FusedAttentionWeights, torch.autograd.Function)
    assert callable(functions.fused_attention_weights_step) and callable(functions.attention_weights_step)
    assert "non-differentiable" in functions.FusedAttentionWeights.__doc__


def _call(l, dtype, C, E_, n_q, n_k, h, d, stats=None, b=None, xe=None, a=None):
    n = ctypes.c_void_p(0)
    return l.graphop_attention_weights(dtype, *([n] * 6), stats or n, b or n, xe or n, a or n, C, E_, n_q, n_k, h, d, n, n)


def test_argument_validation_without_gpu():
    """error code 1 (GRAPHOP_ERR_ARG) and the text, through ctypes with dummy pointers, in the order the header states:
    dtype and sizes, b with xe, NULL stats / a; nothing touches a device"""
    from custom_op_benchmark_amd import _lib
    l = _lib.lib()
    some = ctypes.c_void_p(256)
    err = l.graphop_last_error
    assert _call(l, 7, 4, 10, 5, 5, 2, 8, some, some, some, some) == 1 and b"attention_weights: bad dtype" in err()
    assert _call(l, 2, 4, 10, 5, 5, 2, 8) == 1 and b"attention_weights: bad dtype" in err()
    for sizes in ((-1, 10, 5, 5, 2, 8), (4, -10, 5, 5, 2, 8), (4, 10, -5, 5, 2, 8), (4, 10, 5, -5, 2, 8),
                  (4, 10, 5, 5, 0, 8), (4, 10, 5, 5, 2, -8)):
        assert _call(l, 0, *sizes, some, None, None, some) == 1 and b"attention_weights: negative size" in err()
    for dtype in (0, 1):
        assert _call(l, dtype, 4, 10, 5, 5, 2, 8, some, some, some, some) == 1
        assert b"attention_weights: at most one of b and xe" in err()
        assert _call(l, dtype, 4, 10, 5, 5, 2, 8, None, some, some, None) == 1 and b"at most one of b and xe" in err()
        assert _call(l, dtype, 4, 10, 5, 5, 2, 8, None, None, None, some) == 1 and b"attention_weights: stats is NULL" in err()
        assert _call(l, dtype, 4, 10, 5, 5, 2, 8, None, some, None, some) == 1 and b"stats is NULL" in err()
        assert _call(l, dtype, 4, 10, 5, 5, 2, 8, some, None, some, None) == 1 and b"attention_weights: a is NULL" in err()
    # empty problems are no-ops that never dereference anything
    assert _call(l, 0, 0, 0, 0, 0, 1, 8) == 0
    assert _call(l, 1, 0, 10, 5, 5, 2, 8) == 0          # no chunks
    assert _call(l, 0, 4, 0, 5, 5, 2, 8) == 0           # no edges
    assert _call(l, 0, 4, 10, 0, 5, 2, 8) == 0          # no query rows
    assert _call(l, 1, 4, 10, 5, 5, 2, 0, xe=some) == 0          # d == 0
    # ... but b with xe is refused even then
    assert _call(l, 0, 0, 0, 0, 0, 1, 8, b=some, xe=some) == 1


def test_binding_refusals_without_gpu():
    """the index and value tensors first, then the mode, stats, and b / xe in the words of the ops that take them"""
    from custom_op_benchmark_amd import graphop as ops
    i = torch.zeros(2, dtype=torch.int64)
    v = torch.zeros(2, 4, 8)
    st = torch.zeros(2, 4, 2)
    for mod in (ops, ops.cpp_ext):
        with pytest.raises(RuntimeError, match="row must be a CUDA tensor"):
            mod.attention_weights(i, i, i, i, v, v, st)
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            mod.attention_weights(i, i, i, i, v, v, st, xe=torch.zeros(2, 4, 8))
    fn = "attention_weights"
    with pytest.raises(RuntimeError, match="attention_weights: at most one of b and xe may be given"):
        ops._attn_weights_operands(fn, v, v, st, torch.zeros(2, 4), torch.zeros(2, 4, 8), 2)
    for bad in (torch.zeros(2, 4, 3), torch.zeros(3, 4, 2), torch.zeros(2, 1, 2), torch.zeros(2, 8), torch.zeros(16)):
        with pytest.raises(RuntimeError, match=r"attention_weights: stats must be \(n_q, h, 2\)"):
            ops._attn_weights_operands(fn, v, v, bad, None, None, 2)
    with pytest.raises(RuntimeError, match=r"stats must be \(n_q, h, 2\)"):
        ops._attn_weights_operands(fn, v[:, 0], v[:, 0], st, None, None, 2)          # 2-D Q is one head
    with pytest.raises(RuntimeError, match="expected Q and stats to have the same dtype"):
        ops._attn_weights_operands(fn, v, v, st.double(), None, None, 2)
    with pytest.raises(RuntimeError, match="expected Q and K to have the same dtype"):
        ops._attn_weights_operands(fn, v, v.double(), st, None, None, 2)
    with pytest.raises(RuntimeError, match=r"Q \(n_q,\[h,\]d\) and K \(n_k,\[h,\]d\) expected"):
        ops._attn_weights_operands(fn, v, torch.zeros(2, 4, 16), st, None, None, 2)
    bias = r"attention_weights: b must be \(n_edges\) for 2-D Q / K / V, else \(n_edges, h\)"
    for bad, msg in ((torch.zeros(2, 4, dtype=torch.float64), "expected Q and b to have the same dtype"),
                     (torch.zeros(1, 4), "b must hold one entry per edge id"), (torch.zeros(2), bias),
                     (torch.zeros(2, 3), bias), (torch.zeros(3, 4), bias)):
        with pytest.raises(RuntimeError, match=msg):
            ops._attn_weights_operands(fn, v, v, st, bad, None, 2)
    shape = r"attention_weights: xe must be \(n_edges, d\) for 2-D Q / K / V, else \(n_edges, h, d\)"
    for bad, msg in ((torch.zeros(2, 4, 8, dtype=torch.float64), "expected Q and xe to have the same dtype"),
                     (torch.zeros(1, 4, 8), shape), (torch.zeros(2, 8), shape), (torch.zeros(2, 4, 4), shape),
                     (torch.zeros(2, 4, 16)[:, :, ::2], "xe must be contiguous"),
                     (torch.zeros(2, 4, 8), "xe must be a CUDA tensor")):
        with pytest.raises(RuntimeError, match=msg):
            ops._attn_weights_operands(fn, v, v, st, None, bad, 2)
    assert ops._attn_weights_operands(fn, v, v, st, torch.zeros(2, 4), None, 2) == (4, 8)
    assert ops._attn_weights_operands(fn, v[:, 0], v[:, 0], st[:, :1], torch.zeros(2), None, 2) == (1, 8)


def test_weights_kernels_census():
    """The exact instantiation sets of the k_attn_weights_* kernels (the nine (H, D) pairs; the stream pass per dtype and
    bias; the generic one per dtype), no scratch and no spilled VGPR in any, and names that stay clear of the patterns
    that pin the kernels of the older ops."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources()
    mine = {n: r for n, r in res.items() if "k_attn_weights_" in n}
    fam = {}
    for n, r in mine.items():
        assert not r["spill_vgpr"] and not r["scratch"], (n, r)
        m = re.search(r"graphop::(k_attn_weights_\w+)<(.*)>\(", n)
        assert m, n
        fam.setdefault(m.group(1), {})[m.group(2)] = r
    ty, tf = ("float", "double"), ("false", "true")
    want = {
        "k_attn_weights_norm": {", ".join((t, b)) for t in ty for b in tf},
        "k_attn_weights_xe_f32": {"%d, %d" % p for p in W.HD},
        "k_attn_weights_xe_generic": set(ty),
    }
    assert set(fam) == set(want), sorted(set(fam) ^ set(want))
    for k in want:
        assert set(fam[k]) == want[k], (k, sorted(set(fam[k]) ^ want[k]))
    assert sum(len(v) for v in fam.values()) == len(mine) == 15
    assert not [n for n in mine if "k_attn_edge_" in n or "k_attn_bias_" in n or "k_attn_heads_" in n]
    assert not [n for n in mine if re.search(r"k_attn_(bwd_rows|bwd_wown|fwd_walk)_f32<", n)]
    xe = fam["k_attn_weights_xe_f32"]
    print("k_attn_weights_xe_f32 VGPRs: %d..%d" % (min(r["vgpr"] for r in xe.values()), max(r["vgpr"] for r in xe.values())))
    print("k_attn_weights_* kernels that spill SGPRs:", {n: r["spill_sgpr"] for n, r in mine.items() if r["spill_sgpr"]})
