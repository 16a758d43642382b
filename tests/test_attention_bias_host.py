"""CPU tier of the per-edge score bias of the fused dot-product attention step (graphop_attention_bias_*, DESIGN.md
4.5k): the formulas the kernels implement equal autograd through the float64 reference, b = 0 is the reference without
a bias, a per-row constant in b moves only the row maximum, the library and the bindings expose the ops and validate
their arguments before anything touches a device, and the gfx950 code object keeps every k_attn_bias_* kernel out of
scratch."""
import ctypes
import os
import re
import sys

import pytest
import torch

import attention_bias_reference as B
import attention_dropout_reference as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("attention_bias_forward", "attention_bias_backward")


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
    Q, K, V, dO = (torch.randn(n, h, d, generator=gen, dtype=torch.float64) for n in (n_q, n_k, n_k, n_q))
    b = torch.randn(src.numel(), h, generator=gen, dtype=torch.float64)
    assert n_q != n_k and (torch.bincount(src, minlength=n_q) == 0).any()
    assert torch.unique(torch.stack([src, dst], 1), dim=0).size(0) < src.numel()          # parallel edges
    return src, dst, n_q, n_k, Q, K, V, b, dO


@pytest.mark.parametrize("p", [0.0, 0.6])
@pytest.mark.parametrize("h", [1, 3])
def test_backward_formulas_match_autograd(h, p):
    """o, dQ, dK, dV and db = ds as DESIGN.md 4.5k states them against autograd through the reference layer, in float64"""
    src, dst, n_q, n_k, Q, K, V, b, dO = _case(h)
    seed, offset = 1234567890123, 7
    want = B.reference_step(src, dst, n_q, Q, K, V, b, dO, p, seed, offset)
    mult = A.head_multipliers(src.numpy(), dst.numpy(), 0, h, p, seed, offset) if p > 0 else \
        torch.ones(src.numel(), h, dtype=torch.float64)
    o, D, dQ, dK, dV, db = B.restated(src, dst, n_q, n_k, Q, K, V, b, dO, mult)
    tol = dict(rtol=1e-10, atol=1e-10)
    for name, got in (("o", o), ("dQ", dQ), ("dK", dK), ("dV", dV), ("db", db)):
        torch.testing.assert_close(got, want[name], **tol, msg=lambda m: name + ": " + m)
    # the gradient of b sums to zero over every row where nothing is dropped (a softmax does not see a common shift)
    if p == 0:
        torch.testing.assert_close(torch.zeros(n_q, h, dtype=torch.float64).index_add(0, src, db),
                                   torch.zeros(n_q, h, dtype=torch.float64), **tol)


@pytest.mark.parametrize("p", [0.0, 0.6])
def test_zero_bias_is_the_reference_without_a_bias(p):
    src, dst, n_q, n_k, Q, K, V, b, dO = _case(3, seed=5)
    got = B.reference_step(src, dst, n_q, Q, K, V, torch.zeros_like(b), dO, p, 99, 2)
    want = A.reference_step(src, dst, n_q, Q, K, V, dO, p, 99, 2)
    for k in ("o", "dQ", "dK", "dV", "stats"):
        assert torch.equal(got[k], want[k]), k


def test_a_per_row_constant_moves_only_the_row_maximum():
    src, dst, n_q, n_k, Q, K, V, b, dO = _case(2, seed=7)
    c = torch.randn(n_q, 2, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    base = B.reference_step(src, dst, n_q, Q, K, V, b, dO)
    moved = B.reference_step(src, dst, n_q, Q, K, V, b + c[src], dO)
    torch.testing.assert_close(moved["o"], base["o"], rtol=1e-12, atol=1e-12)
    has = torch.bincount(src, minlength=n_q) > 0
    torch.testing.assert_close(moved["stats"][has][..., 0], (base["stats"][..., 0] + c)[has], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(moved["stats"][..., 1], base["stats"][..., 1], rtol=1e-10, atol=1e-12)


def test_symbols_resolve_in_the_library_and_the_extension():
    from custom_op_benchmark_amd import _ext, _lib, functions, graphop as ops
    l = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES + ("attention_bias_workspace_bytes",):
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
            assert args[4:8] == ["Q", "K", "V", "b"] and args[8:] == tail, doc
        else:
            assert args[8:15] == ["Q", "K", "V", "b", "o", "stats", "dO"] and args[15:] == tail + ["need_db = True"], doc
    assert issubclass(functions.FusedAttentionBias, torch.autograd.Function)
    assert callable(functions.fused_attention_bias_step) and callable(functions.attention_bias_step)
    for text in (functions.FusedAttentionBias.__doc__, ops.attention_bias_forward.__doc__):
        assert "finite" in text and "not a mask" in text and "1 / sqrt(d)" in text
        for use in ("Graphormer", "log w", "node_mul_edge_forward(Q, xe)"):
            assert use in text, use
    assert len(ops.__all__) == 8 and not set(NAMES) & set(ops.__all__)


def _fwd(l, dtype, C, E, n_q, n_k, h, d, p=0.0, seed=0, offset=0, head0=0, b=None, ws=None, ws_bytes=0):
    n = ctypes.c_void_p(0)
    return l.graphop_attention_bias_forward(dtype, *([n] * 7), b or n, n, n, C, E, n_q, n_k, h, d, ws or n, ws_bytes, n, n,
                                            p, seed, offset, head0)


def _bwd(l, dtype, C, C2, E, n_q, n_k, h, d, p=0.0, seed=0, offset=0, head0=0, b=None, ws=None, ws_bytes=0):
    n = ctypes.c_void_p(0)
    return l.graphop_attention_bias_backward(dtype, *([n] * 11), b or n, *([n] * 7), C, C2, E, n_q, n_k, h, d, ws or n,
                                             ws_bytes, n, n, n, p, seed, offset, head0)


def _ws(l, which, dtype, backward, E, n_q, n_k, h, d, *extra):
    out = ctypes.c_int64(-1)
    n = ctypes.c_void_p(0)
    assert getattr(l, which)(dtype, backward, E, n_q, n_k, h, d, n, n, n, *extra, ctypes.byref(out)) == 0
    return out.value


def test_argument_validation_without_gpu():
    from custom_op_benchmark_amd import _lib, graphop as ops
    l = _lib.lib()
    some = ctypes.c_void_p(256)
    for p in (1.0, -0.1, float("nan"), 1.5):
        assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, p, b=some) == 1 and b"p must be in [0, 1)" in l.graphop_last_error()
        assert _bwd(l, 0, 4, 4, 10, 5, 5, 2, 8, p, b=some) == 1 and b"p must be in [0, 1)" in l.graphop_last_error()
    assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, 0.5, seed=2 ** 63, b=some) == 1 and b"seed" in l.graphop_last_error()
    assert _bwd(l, 1, 4, 4, 10, 5, 5, 2, 8, 0.5, seed=2 ** 63, b=some) == 1 and b"seed" in l.graphop_last_error()
    assert _fwd(l, 0, 4, 10, 2 ** 32, 5, 2, 8, 0.5, b=some) == 1 and b"32 bits" in l.graphop_last_error()
    assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, 0.5, head0=-1, b=some) == 1 and b"head0" in l.graphop_last_error()
    assert _bwd(l, 0, 4, 4, 10, 5, 5, 2, 8, 0.0, head0=2 ** 32, b=some) == 1 and b"head0" in l.graphop_last_error()
    # the order: the checks of the undropped entry points, then the dropout arguments, then b
    assert _fwd(l, 7, 0, 0, 0, 0, 1, 8, 1.5) == 1 and b"dtype" in l.graphop_last_error()
    assert _bwd(l, 0, 0, -3, 0, 0, 0, 1, 8, 1.5) == 1 and b"negative" in l.graphop_last_error()
    assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, 1.5) == 1 and b"p must be in [0, 1)" in l.graphop_last_error()
    assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, 0.5) == 1 and b"b is NULL" in l.graphop_last_error()
    assert _bwd(l, 1, 4, 4, 10, 5, 5, 2, 8, 0.0) == 1 and b"b is NULL" in l.graphop_last_error()
    # the workspace: the forward's is that of the other queries; the composed backward (no plans here) holds the arrays
    # of the dropout form without db and one E-sized array fewer with it -- db takes the place of ds
    E, n, h, d = 1000, 50, 2, 8
    for dtype, es in ((0, 4), (1, 8)):
        drop_f = _ws(l, "graphop_attention_dropout_workspace_bytes", dtype, 0, E, n, n, h, d)
        assert _ws(l, "graphop_attention_bias_workspace_bytes", dtype, 0, E, n, n, h, d, 0) == drop_f
        assert _ws(l, "graphop_attention_bias_workspace_bytes", dtype, 0, E, n, n, h, d, 1) == drop_f
        drop = _ws(l, "graphop_attention_dropout_workspace_bytes", dtype, 1, E, n, n, h, d)
        without = _ws(l, "graphop_attention_bias_workspace_bytes", dtype, 1, E, n, n, h, d, 0)
        with_db = _ws(l, "graphop_attention_bias_workspace_bytes", dtype, 1, E, n, n, h, d, 1)
        one = (es * E * h + 255) // 256 * 256
        assert without == drop and with_db == drop - one, (drop, without, with_db, one)
        # ... and the entry points insist on it (plan-less: the composed path)
        assert _bwd(l, dtype, 4, 4, E, n, n, h, d, 0.5, b=some, ws=some, ws_bytes=with_db) == 1
        assert b"attention_bias_workspace_bytes" in l.graphop_last_error()
    # the bindings: the dropout arguments, then b's dtype, length and head count
    i = torch.zeros(2, dtype=torch.int64)
    v = torch.zeros(2, 4, 8)
    st = torch.zeros(2, 4, 2)
    b = torch.zeros(2, 4)
    for kw, msg in ((dict(p=0.5, offset=2 ** 32), "offset"), (dict(p=0.5, offset=-1), "offset"),
                    (dict(p=1.0), r"p must be in \[0, 1\)"), (dict(p=float("nan")), r"p must be in \[0, 1\)"),
                    (dict(p=0.5, seed=2 ** 63), "seed"), (dict(p=0.5, seed=-1), "seed"),
                    (dict(p=0.5, head0=-1), "head0"), (dict(head0=2 ** 32), "head0")):
        with pytest.raises(RuntimeError, match=msg):
            ops.attention_bias_forward(i, i, i, i, v, v, v, b, **kw)
        with pytest.raises(RuntimeError, match=msg):
            ops.attention_bias_backward(i, i, i, i, i, i, i, i, v, v, v, b, v, st, v, **kw)
    for kw, msg in ((dict(p=0.5, offset=2 ** 32), "offset"), (dict(p=1.0), r"p must be in \[0, 1\)"),
                    (dict(p=0.5, seed=-1), "seed"), (dict(head0=-1), "head0")):
        with pytest.raises(RuntimeError, match=msg):
            ops.cpp_ext.attention_bias_forward(i, i, i, i, v, v, v, b, **kw)
        with pytest.raises(RuntimeError, match=msg):
            ops.cpp_ext.attention_bias_backward(i, i, i, i, i, i, i, i, v, v, v, b, v, st, v, **kw)
    # CPU tensors are refused like everywhere else
    with pytest.raises(RuntimeError, match="row must be a CUDA tensor"):
        ops.attention_bias_forward(i, i, i, i, v, v, v, b)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.cpp_ext.attention_bias_backward(i, i, i, i, i, i, i, i, v, v, v, b, v, st, v)
    # b against the graph and the heads: the check both bindings share in wording (graphop._attn_bias)
    for bad, msg in ((torch.zeros(2, 4, dtype=torch.float64), "expected Q and b to have the same dtype"),
                     (torch.zeros(1, 4), "b must hold one entry per edge id"),
                     (torch.zeros(2, 3), r"b must be \(n_edges\) for 2-D Q / K / V, else \(n_edges, h\)"),
                     (torch.zeros(2), r"b must be \(n_edges\) for 2-D Q / K / V, else \(n_edges, h\)"),
                     (torch.zeros(3, 4), r"b must be \(n_edges\) for 2-D Q / K / V, else \(n_edges, h\)")):
        with pytest.raises(RuntimeError, match=msg):
            ops._attn_bias("attention_bias_forward", bad, v, 2, 4)
    with pytest.raises(RuntimeError, match=r"b must be \(n_edges\)"):
        ops._attn_bias("attention_bias_forward", torch.zeros(2, 1), v[:, 0], 2, 1)
    # empty problems are no-ops that never dereference anything
    assert _fwd(l, 0, 0, 0, 0, 0, 1, 8, 0.6) == 0
    assert _fwd(l, 1, 0, 0, 0, 7, 4, 16, 0.6, seed=2 ** 63 - 1, offset=2 ** 32 - 1, head0=4) == 0
    assert _bwd(l, 0, 0, 0, 0, 0, 0, 1, 8, 0.6) == 0
    assert _bwd(l, 1, 0, 0, 0, 0, 0, 3, 8) == 0


def test_bias_kernels_do_not_spill():
    """Every k_attn_bias_* instantiation: no scratch, no spilled VGPR; the chunk-driver backward exists for every
    (L, NV, COL, OWNED, DROP) its twin without a bias has, the forward for every (L, NV, DROP)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources()
    bias = {n: r for n, r in res.items() if "graphop::k_attn_bias_" in n}
    fam = {}
    for n, r in bias.items():
        m = re.search(r"graphop::(k_attn_bias_\w+)<(.*)>\(", n)
        assert m, n
        fam.setdefault(m.group(1), {})[m.group(2)] = r
        assert not r["spill_vgpr"] and not r["scratch"], (n, r)
    assert set(fam) == {"k_attn_bias_add", "k_attn_bias_bwd_rows_f32", "k_attn_bias_fwd_rows_f32", "k_attn_bias_piece_add",
                        "k_attn_bias_piece_fin"}, sorted(fam)
    lnv = ("4, 1", "8, 1", "16, 1", "32, 1", "64, 1", "64, 2", "64, 4")
    tf = ("false", "true")
    assert set(fam["k_attn_bias_bwd_rows_f32"]) == {", ".join((a, c, o, dr)) for a in lnv for c in tf for o in tf for dr in tf}
    assert set(fam["k_attn_bias_fwd_rows_f32"]) == {", ".join((a, dr)) for a in lnv for dr in tf}
    assert set(fam["k_attn_bias_piece_add"]) == set(lnv) == set(fam["k_attn_bias_piece_fin"])
    # the names stay clear of the pattern that pins the kernels without a bias (tests/test_attention_dropout_host.py)
    assert not [n for n in bias if re.search(r"k_attn_(bwd_rows|bwd_wown|fwd_walk)_f32<", n)]
    spilled = {n: r["spill_sgpr"] for n, r in bias.items() if r["spill_sgpr"]}
    print("k_attn_bias_* kernels that spill SGPRs (DESIGN.md 4.5k records them):", spilled)
