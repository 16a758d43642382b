"""CPU tier of the attention dropout of the fused GATv2 layer (graphop_gatv2_attention_dropout_*): the library and both
bindings expose the ops, arguments are validated before anything touches a device, CPU tensors are refused, the new fast
kernels keep their loops in registers, the formulas of include/graphop_hip.h restated in float64 match autograd through
the reference layer, and torch's own fp32 evaluation of that reference sits inside the bounds the GPU tests hold the
kernels to."""
import ctypes
import os
import re
import sys

import pytest
import torch

import dropout_reference as DR
import fused_gatv2_reference as R
import gatv2_dropout_reference as RD
from conftest import ROOT
from test_fused_gatv2_host import _small_case

NAMES = ("gatv2_attention_dropout_forward", "gatv2_attention_dropout_backward")


def test_gatv2_dropout_symbols_resolve_in_the_library_and_the_extension():
    from custom_op_benchmark_amd import _ext, _lib, graphop
    l = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(l, "graphop_" + n) and "graphop_" + n in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 8 and _lib.lib().graphop_abi_version() == 8
    ext = _ext.load()
    assert ext is not None, "graphop_cpp.so not built (run __graft_entry__.build())"
    assert graphop.cpp_ext is ext
    for n in NAMES:
        assert callable(getattr(ext, n)) and hasattr(torch.ops.graphop, n)


def test_gatv2_dropout_ops_are_extra_ops_with_an_autograd_class():
    from custom_op_benchmark_amd import functions, graphop as ops
    for n in NAMES:
        assert n in ops.EXTRA_OPS and callable(getattr(ops, n))
        assert "Tensor att, " in ops._SCHEMAS[n] and "float p=0.0, int seed=0, int offset=0" in ops._SCHEMAS[n]
    assert issubclass(functions.FusedGATv2AttentionDropout, torch.autograd.Function)
    assert callable(functions.fused_gatv2_attention_dropout_step) and callable(functions.gatv2_attention_dropout_step)
    assert len(ops.__all__) == 8 and not set(NAMES) & set(ops.__all__)      # the reference's eight names only
    assert ops.cpp_ext is not None, "graphop_cpp.so not built (run __graft_entry__.build())"
    for n in NAMES:
        assert torch._C.parse_schema("graphop::" + n + ops._SCHEMAS[n]) == getattr(torch.ops.graphop, n).default._schema
        assert all(torch._C._dispatch_has_kernel_for_dispatch_key("graphop::" + n, k)
                   for k in ("CUDA", "CPU"))                           # the CUDA key and the refusing CPU key


def _fwd(l, dtype, C, E, n_l, n_r, h, d, p, seed=0, offset=0):
    n = ctypes.c_void_p(0)
    return l.graphop_gatv2_attention_dropout_forward(dtype, *([n] * 9), C, E, n_l, n_r, h, d, 0.2, p, seed, offset, n,
                                                     n)


def _bwd(l, dtype, Cr, Cc, E, n_l, n_r, h, d, p, seed=0, offset=0, ws_bytes=0):
    n = ctypes.c_void_p(0)
    return l.graphop_gatv2_attention_dropout_backward(dtype, *([n] * 18), ws_bytes, Cr, Cc, E, n_l, n_r, h, d, 0.2, p,
                                                      seed, offset, n, n, n)


def test_gatv2_dropout_argument_validation_without_gpu():
    from custom_op_benchmark_amd import _lib, graphop as ops
    l = _lib.lib()
    for p in (-0.1, 1.0, float("nan"), 1.5):
        assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, p) == 1 and b"p must be in [0, 1)" in l.graphop_last_error()
        assert _bwd(l, 0, 4, 4, 10, 5, 5, 2, 8, p) == 1 and b"p must be in [0, 1)" in l.graphop_last_error()
    assert _fwd(l, 0, 4, 10, 5, 5, 2, 8, 0.5, seed=2 ** 63) == 1 and b"seed" in l.graphop_last_error()
    assert _bwd(l, 1, 4, 4, 10, 5, 5, 2, 8, 0.5, seed=2 ** 63) == 1 and b"seed" in l.graphop_last_error()
    # the counter holds node ids as 32-bit words
    assert _fwd(l, 0, 4, 10, 2 ** 32, 5, 2, 8, 0.5) == 1 and b"32 bits" in l.graphop_last_error()
    assert _bwd(l, 0, 4, 4, 10, 5, 2 ** 32, 2, 8, 0.5) == 1 and b"32 bits" in l.graphop_last_error()
    # the checks the undropped entry points make come first
    assert _fwd(l, 7, 0, 0, 0, 0, 1, 8, 0.5) == 1 and b"dtype" in l.graphop_last_error()
    assert _bwd(l, 7, 0, 0, 0, 0, 0, 1, 8, 0.5) == 1 and b"dtype" in l.graphop_last_error()
    assert _fwd(l, 0, -1, 0, 0, 0, 1, 8, 0.5) == 1 and b"negative" in l.graphop_last_error()
    assert _bwd(l, 0, 0, -3, 0, 0, 0, 1, 8, 0.5) == 1 and b"negative" in l.graphop_last_error()
    for h, d in ((0, 8), (1, 0)):
        assert _fwd(l, 0, 0, 0, 0, 0, h, d, 0.5) == 1 and b"negative" in l.graphop_last_error()
    # the workspace rule of gatv2_attention_backward: one value below n_l * h * 4 + min(ceil(n_row_chunks / 16), 8192) *
    # h * d values is refused, with and without dropout
    need = 5 * 2 * 4 + 7 * 2 * 8                                    # 100 row chunks -> 7 rows of partials
    assert need == ops._gatv2_attention_workspace_values(5, 100, 2, 8)
    for p in (0.0, 0.6):
        for dtype, es in ((0, 4), (1, 8)):
            assert _bwd(l, dtype, 100, 4, 10, 5, 5, 2, 8, p, ws_bytes=(need - 1) * es) == 1
            assert b"workspace" in l.graphop_last_error()
            # the full size passes this check and fails on the next one (a NULL table) instead
            assert _bwd(l, dtype, 100, 4, 10, 5, 5, 2, 8, p, ws_bytes=need * es) == 1
            assert b"workspace" not in l.graphop_last_error() and b"NULL" in l.graphop_last_error()
    # the C ABI takes offset as a uint32_t: the range check is the bindings'
    i = torch.zeros(2, dtype=torch.int64)
    f, a, st = torch.zeros(2, 4), torch.zeros(4), torch.zeros(2, 1, 2)
    for kw, msg in ((dict(p=0.5, offset=2 ** 32), "offset"), (dict(p=0.5, offset=-1), "offset"),
                    (dict(p=1.0), r"p must be in \[0, 1\)"), (dict(p=float("nan")), r"p must be in \[0, 1\)"),
                    (dict(p=0.5, seed=2 ** 63), "seed"), (dict(p=0.5, seed=-1), "seed")):
        with pytest.raises(RuntimeError, match=msg):
            ops.gatv2_attention_dropout_forward(i, i, i, i, f, f, a, 0.2, **kw)
        with pytest.raises(RuntimeError, match=msg):
            ops.gatv2_attention_dropout_backward(i, i, i, i, i, i, i, i, f, f, a, f, st, f, 0.2, **kw)
    for kw, msg in ((dict(p=0.5, offset=2 ** 32), "offset"), (dict(p=1.0), r"p must be in \[0, 1\)"),
                    (dict(p=0.5, seed=-1), "seed")):
        with pytest.raises(RuntimeError, match=msg):
            ops.cpp_ext.gatv2_attention_dropout_forward(i, i, i, i, f, f, a, 0.2, **kw)
        with pytest.raises(RuntimeError, match=msg):
            ops.cpp_ext.gatv2_attention_dropout_backward(i, i, i, i, i, i, i, i, f, f, a, f, st, f, 0.2, **kw)
    # empty problems are no-ops that never dereference anything
    assert _fwd(l, 0, 0, 0, 0, 0, 1, 8, 0.6) == 0
    assert _fwd(l, 1, 0, 0, 0, 7, 4, 16, 0.6, seed=2 ** 63 - 1, offset=2 ** 32 - 1) == 0
    assert _bwd(l, 0, 0, 0, 0, 0, 0, 1, 8, 0.6) == 0
    assert _bwd(l, 1, 0, 0, 0, 0, 0, 8, 32, 0.0) == 0


def test_gatv2_dropout_cpu_tensors_are_refused():
    from custom_op_benchmark_amd import graphop as ops
    i = torch.zeros(2, dtype=torch.int64)
    f, a, st = torch.zeros(2, 4), torch.zeros(4), torch.zeros(2, 1, 2)
    with pytest.raises(RuntimeError, match="row must be a CUDA tensor"):
        ops.gatv2_attention_dropout_forward(i, i, i, i, f, f, a, 0.2, 0.5, 1, 0)
    with pytest.raises(RuntimeError, match="row must be a CUDA tensor"):
        ops.gatv2_attention_dropout_backward(i, i, i, i, i, i, i, i, f, f, a, f, st, f, 0.2, 0.5, 1, 0)
    with pytest.raises(RuntimeError, match="no CPU implementation|must be a CUDA tensor"):
        torch.ops.graphop.gatv2_attention_dropout_forward(i, i, i, i, f, f, a, 0.2, 0.5, 1, 0)
    with pytest.raises(RuntimeError, match="no CPU implementation|must be a CUDA tensor"):
        torch.ops.graphop.gatv2_attention_dropout_backward(i, i, i, i, i, i, i, i, f, f, a, f, st, f, 0.1, 0.5, 1, 0)


def test_gatv2_dropout_fast_kernels_do_not_spill():
    """Every fast dropout instantiation keeps its loop in registers: no spill, no scratch.  9 (h, d) pairs of the forward,
    9 x {owned, shared} of the row and the column pass; the forward's merge of a long segment stays within 17 KB of LDS."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources()
    fwd = {n: r for n, r in res.items() if re.search(r"k_gv2drop_fwd_f32<\d+, \d+>\(", n)}
    row = {n: r for n, r in res.items() if re.search(r"k_gv2drop_bwd_row_f32<\d+, \d+, (true|false)>\(", n)}
    col = {n: r for n, r in res.items() if re.search(r"k_gv2drop_bwd_col_f32<\d+, \d+, (true|false)>\(", n)}
    assert (len(fwd), len(row), len(col)) == (9, 18, 18), sorted(n for n in res if "k_gv2drop_" in n)
    for h, d in R.FAST:
        assert any("k_gv2drop_fwd_f32<%d, %d>(" % (h, d) in n for n in fwd), (h, d)
        for owned in ("true", "false"):
            assert any("k_gv2drop_bwd_row_f32<%d, %d, %s>(" % (h, d, owned) in n for n in row), (h, d, owned)
            assert any("k_gv2drop_bwd_col_f32<%d, %d, %s>(" % (h, d, owned) in n for n in col), (h, d, owned)
    fast = {**fwd, **row, **col}
    assert len(fast) == len([n for n in res if "k_gv2drop_" in n])           # no dropout kernel left out
    bad = {n: r for n, r in fast.items() if r["spill_vgpr"] or r["spill_sgpr"] or r["scratch"]}
    assert not bad, "\n".join("%s: %r" % kv for kv in sorted(bad.items()))
    assert max(r["lds"] for r in fwd.values()) <= 17 * 1024


@pytest.mark.parametrize("p", [0.1, 0.6, 0.9])
@pytest.mark.parametrize("slope", [0.2, -0.1])
def test_gatv2_dropout_backward_formulas_match_autograd(slope, p):
    """stats, o, D, da, ds and the three sums as include/graphop_hip.h states them, in float64, against autograd through
    the reference layer, on the small graph of the undropped formula test (empty rows, exact z == 0 ties, a row with
    |s| ~ 50, parallel edges, which share one decision).  At p >= 0.6 some non-empty (row, head) loses every edge: its o
    and dxl are exactly zero, its stats still those of its scores."""
    src, dst, n_l, xl, xr, att, dO = _small_case()
    h = xl.size(1)
    seed, offset = 1234567890123, 7
    g = type("G", (), dict(src=src, dst=dst, n_src=n_l))()
    want = RD.reference(g, xl, xr, att, dO, slope, p, seed, offset)
    mult = DR.multipliers(src.numpy(), dst.numpy(), h, p, seed, offset)
    assert torch.unique(torch.stack([src, dst], 1), dim=0).size(0) < src.numel()       # parallel edges
    got = RD.restated(src, dst, n_l, xl, xr, att, dO, slope, mult)
    gone = DR.fully_dropped_rows(src, dst, n_l, h, p, seed, offset)
    if p >= 0.6:
        assert gone.any()
    assert not got[0][gone].any() and not got[2][gone].any() and not want[0][gone].any()
    assert bool((got[1][gone][:, 0] > -1e9).all()) and bool((got[1][gone][:, 1] > 0).all())
    # the statistics do not see the dropout
    torch.testing.assert_close(got[1], R.restated(src, dst, n_l, xl, xr, att, dO, slope)[1], rtol=0, atol=0)
    for name, x, y in zip(("o", "stats", "dxl", "dxr", "datt"), got, want):
        torch.testing.assert_close(x, y, rtol=1e-12, atol=1e-12, msg=lambda msg: name + ": " + msg)


def test_gatv2_dropout_fp32_reference_sits_inside_the_gpu_bounds():
    """torch's own fp32 evaluation of the dropout reference against the float64 one on the two irregular graphs of the GPU
    tests: o, stats, dxl and dxr inside rtol = 1e-4 / atol = 1e-5 / (1 - p), datt inside 1e-6 * S.  The inputs do not
    strain the bounds the kernels are held to.  Measured: o 0.04, stats 0.01, dxl 0.09, dxr 0.07 of the bound, datt 4.7e-8 * S."""
    worst = dict(o=0.0, stats=0.0, dxl=0.0, dxr=0.0, datt=0.0)
    for cs in (3, 32):
        g = R.irregular_graph(cs)
        for h, d in ((1, 64), (4, 16), (8, 32), (3, 8)):
            x = R.inputs(g, h, d, seed=h + d + cs)
            for p in (0.1, 0.5, 0.6, 0.9):
                seed, offset = (0, 0) if p == 0.6 else (1234567890123, 7)
                want = RD.reference(g, *x, 0.2, p, seed, offset)
                got = RD.reference(g, *x, 0.2, p, seed, offset, dtype=torch.float32)
                tol, K = RD.tol(torch.float32, p)
                for name, a, b in zip(("o", "stats", "dxl", "dxr"), got, want):
                    assert a.dtype == torch.float32
                    worst[name] = max(worst[name], R.ratio(a, b, tol))
                worst["datt"] = max(worst["datt"], R.datt_ratio(got[4], want[4], want[5]))
            print("chunk %d (%d, %d): %s" % (cs, h, d, ", ".join("%s %.3g" % kv for kv in worst.items())))
    print("worst: o %.3f, stats %.3f, dxl %.3f, dxr %.3f of the bound; datt %.3g * S" % (
        worst["o"], worst["stats"], worst["dxl"], worst["dxr"], worst["datt"]))
    assert max(worst[n] for n in ("o", "stats", "dxl", "dxr")) <= 1.0, worst
    assert worst["datt"] <= R.K32, worst
