"""CPU tier of the fused dot-product attention step with edge features (graphop_attention_edge_*): the
formulas the kernels implement equal autograd through the float64 reference, the library and the bindings expose the
ops and validate their arguments before anything touches a device, the gfx950 code object holds exactly the
k_attn_edge_* instantiations the op launches and keeps every one out of scratch, and the inputs the GPU tier uses are
ones on which torch's own fp32 arithmetic stays within half of that tier's bounds."""
import ctypes
import os
import re
import sys

import pytest
import torch

import attention_dropout_reference as A
import attention_edge_reference as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("attention_edge_forward", "attention_edge_backward")


def _small_graph(gen, n_q=23, n_k=17):
    """rectangular, rows without edges (every fifth), parallel edges (the diagonal is added twice)"""
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
    assert n_q != n_k and (torch.bincount(src, minlength=n_q) == 0).any()
    assert torch.unique(torch.stack([src, dst], 1), dim=0).size(0) < src.numel()          # parallel edges
    return src, dst, n_q, n_k, Q, K, V, xe, dO


@pytest.mark.parametrize("p", [0.0, 0.6])
@pytest.mark.parametrize("h", [1, 3])
def test_restated_gradients_match_autograd(h, p):
    """o, dQ, dK, dV and dxe = ds Q_i + a m dO_i as DESIGN.md 4.5m states them against autograd through the reference
    layer, in float64 at 1e-12; parallel edges have each their own xe row and gradient"""
    src, dst, n_q, n_k, Q, K, V, xe, dO = _case(h)
    seed, offset = 1234567890123, 7
    want = E.reference_step(src, dst, n_q, Q, K, V, xe, dO, p, seed, offset)
    mult = A.head_multipliers(src.numpy(), dst.numpy(), 0, h, p, seed, offset) if p > 0 else \
        torch.ones(src.numel(), h, dtype=torch.float64)
    o, D, dQ, dK, dV, dxe = E.restated(src, dst, n_q, n_k, Q, K, V, xe, dO, mult)
    for name, got in (("o", o), ("dQ", dQ), ("dK", dK), ("dV", dV), ("dxe", dxe)):
        torch.testing.assert_close(got.reshape(want[name].shape), want[name], rtol=1e-12, atol=1e-12,
                                   msg=lambda m: name + ": " + m)
    pair = torch.stack([src, dst], 1)
    twin = (pair[:-1] == pair[-1]).all(1).nonzero()[0, 0]          # the last edge is a parallel one
    assert not torch.equal(want["dxe"][twin], want["dxe"][-1])
    empty = torch.bincount(src, minlength=n_q) == 0
    assert not want["o"][empty].any() and (want["stats"][empty] == torch.tensor([-1e9, 0.0], dtype=torch.float64)).all()


def test_zero_edge_rows_give_the_op_without_them():
    src, dst, n_q, n_k, Q, K, V, xe, dO = _case(3, seed=5)
    got = E.reference_step(src, dst, n_q, Q, K, V, torch.zeros_like(xe), dO, 0.6, 99, 2)
    want = A.reference_step(src, dst, n_q, Q, K, V, dO, 0.6, 99, 2)
    for k in ("o", "dQ", "dK", "dV"):
        assert torch.equal(got[k], want[k]), k


def test_symbols_resolve_in_the_library_and_the_extension():
    from custom_op_benchmark_amd import _ext, _lib, functions, graphop as ops
    l = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES + ("attention_edge_workspace_bytes",):
        assert hasattr(l, "graphop_" + n) and "graphop_" + n in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 8 and _lib.lib().graphop_abi_version() == 8        # additive: the ABI number stays
    ext = _ext.load()
    assert ext is not None, "graphop_cpp.so not built (run __graft_entry__.build())"
    for n in NAMES:
        assert callable(getattr(ext, n)) and callable(getattr(ops, n))
        assert n in ops.EXTRA_OPS and n not in ops._SCHEMAS and not hasattr(torch.ops.graphop, n)
        doc = getattr(ext, n).__doc__.splitlines()[0]
        args = [a.split(":")[0] + (a[a.index(" = "):] if " = " in a else "") for a in doc[doc.index("(") + 1:doc.rindex(") -> ")].split(", ")]
        tail = ["p = 0.0", "seed = 0", "offset = 0", "head0 = 0"]
        if n.endswith("forward"):
            assert args[4:8] == ["Q", "K", "V", "xe"] and args[8:] == tail, doc
        else:
            assert args[8:15] == ["Q", "K", "V", "xe", "o", "stats", "dO"] and args[15:] == tail + ["need_dxe = True"], doc
    assert issubclass(functions.FusedAttentionEdge, torch.autograd.Function)
    assert callable(functions.fused_attention_edge_step) and callable(functions.attention_edge_step)
    # the docstrings of the bias op no longer send the value-side term to a bias
    for text in (functions.FusedAttentionBias.__doc__, ops.attention_bias_forward.__doc__):
        assert "value" in text and ("FusedAttentionEdge" in text or "attention_edge_forward" in text)
    assert len(ops.__all__) == 8 and not set(NAMES) & set(ops.__all__)


def _fwd(l, dtype, C, E_, n_q, n_k, h, d, p=0.0, seed=0, offset=0, head0=0, xe=None, ws=None, ws_bytes=0):
    n = ctypes.c_void_p(0)
    return l.graphop_attention_edge_forward(dtype, *([n] * 7), xe or n, n, n, C, E_, n_q, n_k, h, d, ws or n, ws_bytes, n, n,
                                            p, seed, offset, head0)


def _bwd(l, dtype, C, C2, E_, n_q, n_k, h, d, p=0.0, seed=0, offset=0, head0=0, xe=None, ws=None, ws_bytes=0):
    n = ctypes.c_void_p(0)
    return l.graphop_attention_edge_backward(dtype, *([n] * 11), xe or n, *([n] * 7), C, C2, E_, n_q, n_k, h, d, ws or n,
                                             ws_bytes, n, n, n, p, seed, offset, head0)


def _ws(l, dtype, backward, E_, n_q, n_k, h, d):
    out = ctypes.c_int64(-1)
    n = ctypes.c_void_p(0)
    assert l.graphop_attention_edge_workspace_bytes(dtype, backward, E_, n_q, n_k, h, d, n, n, n, ctypes.byref(out)) == 0
    return out.value


def test_argument_validation_without_gpu():
    """error code 1 (GRAPHOP_ERR_ARG) and the text, through ctypes with dummy pointers: nothing touches a device"""
    from custom_op_benchmark_amd import _lib
    l = _lib.lib()
    some = ctypes.c_void_p(256)
    err = l.graphop_last_error
    # bad dtype
    assert _fwd(l, 7, 4, 10, 5, 5, 2, 8, xe=some) == 1 and b"attention_edge_forward: bad dtype" in err()
    assert _bwd(l, 2, 4, 4, 10, 5, 5, 2, 8, xe=some) == 1 and b"attention_edge_backward: bad dtype" in err()
    assert _bwd(l, 0, 0, -3, 0, 0, 0, 1, 8) == 1 and b"negative" in err()
    # p out of range
    for p in (1.0, -0.1, float("nan"), 1.5):
        assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, p, xe=some) == 1 and b"p must be in [0, 1)" in err()
        assert _bwd(l, 0, 4, 4, 10, 5, 5, 2, 8, p, xe=some) == 1 and b"p must be in [0, 1)" in err()
    assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, 0.5, seed=2 ** 63, xe=some) == 1 and b"seed" in err()
    assert _fwd(l, 0, 4, 10, 2 ** 32, 5, 2, 8, 0.5, xe=some) == 1 and b"32 bits" in err()
    # head0 out of range, also at p == 0
    assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, 0.5, head0=-1, xe=some) == 1 and b"head0 must be in [0, 2^32)" in err()
    assert _bwd(l, 0, 4, 4, 10, 5, 5, 2, 8, 0.0, head0=2 ** 32, xe=some) == 1 and b"head0 must be in [0, 2^32)" in err()
    # NULL xe, after the other checks: dtype, then p, then xe
    assert _fwd(l, 7, 4, 10, 5, 5, 2, 8, 1.5) == 1 and b"dtype" in err()
    assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, 1.5) == 1 and b"p must be in [0, 1)" in err()
    assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, 0.5) == 1 and b"attention_edge_forward: xe is NULL" in err()
    assert _bwd(l, 1, 4, 4, 10, 5, 5, 2, 8, 0.0) == 1 and b"attention_edge_backward: xe is NULL" in err()
    # short workspace: plan-less, the generic backward wants P (n_q, h, 4) in the op's dtype; the forward wants none
    E_, n, h, d = 1000, 50, 2, 8
    for dtype, es in ((0, 4), (1, 8)):
        assert _ws(l, dtype, 0, E_, n, n, h, d) == 0
        need = _ws(l, dtype, 1, E_, n, n, h, d)
        assert need == (es * 4 * n * h + 255) // 256 * 256
        assert _bwd(l, dtype, 4, 4, E_, n, n, h, d, 0.5, xe=some, ws=some, ws_bytes=need - 1) == 1
        assert b"attention_edge_backward: workspace of %d bytes needed (graphop_attention_edge_workspace_bytes)" % need in err()
        assert _bwd(l, dtype, 4, 4, E_, n, n, h, d, 0.5, xe=some, ws=None, ws_bytes=need) == 1 and b"workspace" in err()
    out = ctypes.c_int64(-1)
    n0 = ctypes.c_void_p(0)
    assert l.graphop_attention_edge_workspace_bytes(5, 1, 10, 5, 5, 2, 8, n0, n0, n0, ctypes.byref(out)) == 1 and b"dtype" in err()
    assert l.graphop_attention_edge_workspace_bytes(0, 1, 10, 5, 5, 2, 8, n0, n0, n0, None) == 1 and b"bytes_out" in err()
    # empty problems are no-ops that never dereference anything
    assert _fwd(l, 0, 0, 0, 0, 0, 1, 8, 0.6) == 0
    assert _fwd(l, 1, 0, 0, 0, 7, 4, 16, 0.6, seed=2 ** 63 - 1, offset=2 ** 32 - 1, head0=4) == 0
    assert _fwd(l, 0, 4, 10, 0, 5, 2, 8, xe=some) == 0          # no query rows
    assert _bwd(l, 0, 0, 0, 0, 0, 0, 1, 8, 0.6) == 0
    assert _bwd(l, 1, 0, 0, 0, 0, 0, 3, 8) == 0
    assert _bwd(l, 0, 4, 4, 10, 5, 5, 2, 0) == 0                # d == 0: xe may be NULL


def test_binding_refusals_without_gpu():
    """the dropout arguments first, then the tensors; xe is checked once per binding, in the same words"""
    from custom_op_benchmark_amd import graphop as ops
    i = torch.zeros(2, dtype=torch.int64)
    v = torch.zeros(2, 4, 8)
    st = torch.zeros(2, 4, 2)
    xe = torch.zeros(2, 4, 8)
    for kw, msg in ((dict(p=0.5, offset=2 ** 32), "offset"), (dict(p=1.0), r"p must be in \[0, 1\)"),
                    (dict(p=float("nan")), r"p must be in \[0, 1\)"), (dict(p=0.5, seed=-1), "seed"),
                    (dict(p=0.5, head0=-1), "head0"), (dict(head0=2 ** 32), "head0")):
        for mod in (ops, ops.cpp_ext):
            with pytest.raises(RuntimeError, match=msg):
                mod.attention_edge_forward(i, i, i, i, v, v, v, xe, **kw)
            with pytest.raises(RuntimeError, match=msg):
                mod.attention_edge_backward(i, i, i, i, i, i, i, i, v, v, v, xe, v, st, v, **kw)
    for mod in (ops, ops.cpp_ext):
        with pytest.raises(RuntimeError, match="row must be a CUDA tensor"):
            mod.attention_edge_forward(i, i, i, i, v, v, v, xe)
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            mod.attention_edge_backward(i, i, i, i, i, i, i, i, v, v, v, xe, v, st, v)
    # xe against the graph and Q (graphop._attn_edge_rows; torch_ext.cpp's check_attn_edge_rows has the same order and
    # words, reached on the GPU tier): dtype, shape, contiguity, device
    shape = r"xe must be \(n_edges, d\) for 2-D Q / K / V, else \(n_edges, h, d\)"
    for bad, msg in ((torch.zeros(2, 4, 8, dtype=torch.float64), "expected Q and xe to have the same dtype"),
                     (torch.zeros(1, 4, 8), shape), (torch.zeros(3, 4, 8), shape), (torch.zeros(2, 4), shape),
                     (torch.zeros(2, 8), shape), (torch.zeros(2, 4, 4), shape), (torch.zeros(2, 3, 8), shape),
                     (torch.zeros(2, 4, 16)[:, :, ::2], "xe must be contiguous"),
                     (torch.zeros(4, 2, 8).transpose(0, 1), "xe must be contiguous"),
                     (torch.zeros(2, 4, 8), "xe must be a CUDA tensor")):
        with pytest.raises(RuntimeError, match=msg):
            ops._attn_edge_rows("attention_edge_forward", bad, v, 2)
    with pytest.raises(RuntimeError, match=shape):
        ops._attn_edge_rows("attention_edge_forward", torch.zeros(2, 1, 8), v[:, 0], 2)          # 2-D Q wants 2-D xe


def test_edge_kernels_census():
    """The exact instantiation sets of the k_attn_edge_* kernels (nine (H, D) pairs x the template booleans; the generic
    ones per dtype), no scratch and no spilled VGPR in any, and names that stay clear of the patterns that pin the
    kernels of the ops without edge rows."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources()
    edge = {n: r for n, r in res.items() if "k_attn_edge_" in n}
    fam = {}
    for n, r in edge.items():
        assert not r["spill_vgpr"] and not r["scratch"], (n, r)
        m = re.search(r"graphop::(k_attn_edge_\w+)<(.*)>\(", n)
        if m:
            fam.setdefault(m.group(1), {})[m.group(2)] = r
        else:
            assert re.search(r"graphop::k_attn_edge_piece_max\(", n), n
            fam.setdefault("k_attn_edge_piece_max", {})[""] = r
    hd = ["%d, %d" % p for p in E.HD]
    tf = ("false", "true")
    ty = ("float", "double")
    want = {
        "k_attn_edge_fwd_rows_f32": {", ".join((a, dr)) for a in hd for dr in tf},
        "k_attn_edge_bwd_rows_f32": {", ".join((a, c, o, dr)) for a in hd for c in tf for o in tf for dr in tf},
        "k_attn_edge_pack": {", ".join((a, s)) for a in hd for s in tf},
        "k_attn_edge_piece_add": set(hd), "k_attn_edge_piece_fin": set(hd), "k_attn_edge_piece_max": {""},
        "k_attn_edge_stats_generic": {", ".join((t, s)) for t in ty for s in tf},
        "k_attn_edge_fwd_generic": {", ".join((t, s)) for t in ty for s in tf},
        "k_attn_edge_bwd_row_generic": {", ".join((t, s)) for t in ty for s in tf},
        "k_attn_edge_bwd_col_generic": {", ".join((t, s)) for t in ty for s in tf},
        "k_attn_edge_stats_init_generic": set(ty), "k_attn_edge_stats_fin_generic": set(ty),
        "k_attn_edge_pack_generic": set(ty),
    }
    assert set(fam) == set(want), sorted(set(fam) ^ set(want))
    for k in want:
        assert set(fam[k]) == want[k], (k, sorted(set(fam[k]) ^ want[k]))
    assert sum(len(v) for v in fam.values()) == len(edge) == 149
    assert not [n for n in edge if "k_attn_heads_" in n or "k_attn_bias_" in n]
    assert not [n for n in edge if re.search(r"k_attn_(bwd_rows|bwd_wown|fwd_walk)_f32<", n)]
    rows = {n: r for n, r in edge.items() if "_rows_f32<" in n}
    print("k_attn_edge_*_rows_f32 VGPRs: %d..%d" % (min(r["vgpr"] for r in rows.values()), max(r["vgpr"] for r in rows.values())))
    print("k_attn_edge_* kernels that spill SGPRs (DESIGN.md 4.5m records them):",
          {n: r["spill_sgpr"] for n, r in edge.items() if r["spill_sgpr"]})


@pytest.mark.parametrize("name", sorted(E.INPUT_SETS))
def test_input_condition(name):
    """Torch's own float32 evaluation of the reference, against the float64 one, stays within 0.5 of the GPU tier's
    bounds (E.tol) on every input set that tier uses, with and without dropout: the bounds leave a kernel that sums in
    another order the other half."""
    g, inp = E.input_set(name)
    src, dst = g.src, g.dst
    for p, seed, offset in (E.NONE, E.DROP):
        want = E.reference_step(src, dst, g.n_src, *inp, p, seed, offset)
        got = E.reference_step(src, dst, g.n_src, *inp, p, seed, offset, dtype=torch.float32)
        t = E.tol(torch.float32, p)
        has = torch.bincount(src, minlength=g.n_src) > 0
        ratios = {k: E.error_ratio(got[k], want[k], **t) for k in E.KEYS}
        ratios["stats"] = E.error_ratio(got["stats"][has], want["stats"][has], **E.tol(torch.float32))
        print(name, "p=%g" % p, {k: round(v, 3) for k, v in ratios.items()})
        assert max(ratios.values()) <= 0.5, (name, p, ratios)
        assert float(E.edge_scores(src, dst, *inp[:2], inp[3]).abs().max()) < 30
