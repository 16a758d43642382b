"""CPU tier of the fused GATv2 attention layer (graphop_gatv2_attention_*): the library and both bindings expose the op,
arguments are validated before anything touches a device, CPU tensors are refused, the fast kernels keep their loops in
registers, the backward formulas of include/graphop_hip.h restated in float64 match autograd through the reference layer,
and torch's own fp32 evaluation of that reference sits inside the bounds the GPU tests hold the kernels to."""
import ctypes
import os
import re
import sys

import pytest
import torch

import fused_gatv2_reference as R
from conftest import ROOT
from gatv2_reference import gatv2_layer

NAMES = ("gatv2_attention_forward", "gatv2_attention_backward")


def test_fused_gatv2_symbols_resolve_in_the_library_and_the_extension():
    from custom_op_benchmark_amd import _ext, _lib, graphop
    l = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(l, "graphop_" + n) and "graphop_" + n in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 8 and _lib.lib().graphop_abi_version() == 8
    ext = _ext.load()
    if ext is None:
        pytest.skip("graphop_cpp.so not built (run __graft_entry__.build())")
    assert graphop.cpp_ext is ext
    for n in NAMES:
        assert callable(getattr(ext, n)) and hasattr(torch.ops.graphop, n)


def test_fused_gatv2_ops_are_extra_ops_with_an_autograd_class():
    from custom_op_benchmark_amd import functions, graphop as ops
    for n in NAMES:
        assert n in ops.EXTRA_OPS and callable(getattr(ops, n))
        assert "float negative_slope=0.2" in ops._SCHEMAS[n] and "Tensor att" in ops._SCHEMAS[n]
    assert issubclass(functions.FusedGATv2Attention, torch.autograd.Function)
    assert callable(functions.fused_gatv2_attention_step)
    assert len(ops.__all__) == 8 and not set(NAMES) & set(ops.__all__)      # the reference's eight names only
    assert ops.cpp_ext is not None, "graphop_cpp.so not built (run __graft_entry__.build())"
    for n in NAMES:
        assert torch._C.parse_schema("graphop::" + n + ops._SCHEMAS[n]) == getattr(torch.ops.graphop, n).default._schema
        assert all(torch._C._dispatch_has_kernel_for_dispatch_key("graphop::" + n, k)
                   for k in ("CUDA", "CPU"))                           # the CUDA key and the refusing CPU key


def test_fused_gatv2_workspace_helper_is_the_headers_minimum():
    """n_l * h * 4 values for the packed row table plus min(ceil(n_row_chunks / 16), 8192) * h * d for the datt partials"""
    from custom_op_benchmark_amd import graphop as ops
    h, d = 2, 32
    got = [ops._gatv2_attention_workspace_values(n_l, c, h, d)
           for n_l, c in ((0, 0), (5, 0), (5, 1), (7, 16), (7, 17), (1000, 16 * 8192), (3, 10 ** 7))]
    assert got == [0, 40, 40 + 64, 56 + 64, 56 + 128, 8000 + 8192 * 64, 24 + 8192 * 64]
    text = open(os.path.join(ROOT, "include", "graphop_hip.h")).read()
    assert "n_l * h * 4 values" in text and "min(ceil(n_row_chunks / 16), 8192) * h * d values" in text


def _fwd(l, dtype, C, E, n_l, n_r, h, d):
    n = ctypes.c_void_p(0)
    return l.graphop_gatv2_attention_forward(dtype, n, n, n, n, n, n, n, n, n, C, E, n_l, n_r, h, d, 0.2, n, n)


def _bwd(l, dtype, Cr, Cc, E, n_l, n_r, h, d, ws_bytes=0):
    n = ctypes.c_void_p(0)
    return l.graphop_gatv2_attention_backward(dtype, *([n] * 8), *([n] * 10), ws_bytes, Cr, Cc, E, n_l, n_r, h, d, 0.2,
                                              n, n, n)


def test_fused_gatv2_argument_validation_without_gpu():
    from custom_op_benchmark_amd import _lib
    l = _lib.lib()
    assert _fwd(l, 7, 0, 0, 0, 0, 1, 8) == 1 and b"dtype" in l.graphop_last_error()
    assert _bwd(l, 7, 0, 0, 0, 0, 0, 1, 8) == 1 and b"dtype" in l.graphop_last_error()
    assert _fwd(l, 0, -1, 0, 0, 0, 1, 8) == 1 and b"negative" in l.graphop_last_error()
    assert _fwd(l, 1, 0, 0, 0, -2, 1, 8) == 1 and b"negative" in l.graphop_last_error()
    assert _bwd(l, 1, 0, -3, 0, 0, 0, 1, 8) == 1 and b"negative" in l.graphop_last_error()
    assert _bwd(l, 0, 0, 0, -1, 0, 0, 1, 8) == 1 and b"negative" in l.graphop_last_error()
    for h, d in ((0, 8), (1, 0)):
        assert _fwd(l, 0, 0, 0, 0, 0, h, d) == 1 and b"negative" in l.graphop_last_error()
        assert _bwd(l, 0, 0, 0, 0, 0, 0, h, d) == 1 and b"negative" in l.graphop_last_error()
    # a workspace one value below n_l * h * 4 + min(ceil(n_row_chunks / 16), 8192) * h * d values is refused
    need = 5 * 2 * 4 + 7 * 2 * 8                                    # 100 row chunks -> 7 rows of partials
    for dtype, es in ((0, 4), (1, 8)):
        assert _bwd(l, dtype, 100, 4, 10, 5, 5, 2, 8, ws_bytes=(need - 1) * es) == 1
        assert b"workspace" in l.graphop_last_error()
        # the full size passes this check and fails on the next one (a NULL table) instead
        assert _bwd(l, dtype, 100, 4, 10, 5, 5, 2, 8, ws_bytes=need * es) == 1
        assert b"workspace" not in l.graphop_last_error() and b"NULL" in l.graphop_last_error()
    need = 5 * 2 * 4 + 8192 * 2 * 8                                 # the partial rows are capped at 8192
    assert _bwd(l, 0, 10 ** 7, 4, 10, 5, 5, 2, 8, ws_bytes=(need - 1) * 4) == 1 and b"workspace" in l.graphop_last_error()
    assert _bwd(l, 0, 10 ** 7, 4, 10, 5, 5, 2, 8, ws_bytes=need * 4) == 1 and b"NULL" in l.graphop_last_error()
    # empty problems are no-ops that never dereference anything
    assert _fwd(l, 0, 0, 0, 0, 0, 1, 8) == 0
    assert _fwd(l, 1, 0, 0, 0, 7, 4, 16) == 0
    assert _bwd(l, 0, 0, 0, 0, 0, 0, 1, 8) == 0
    assert _bwd(l, 1, 0, 0, 0, 0, 0, 8, 32) == 0


def test_fused_gatv2_cpu_tensors_are_refused():
    from custom_op_benchmark_amd import graphop as ops
    i = torch.zeros(2, dtype=torch.int64)
    f = torch.zeros(2, 4)
    a = torch.zeros(4)
    st = torch.zeros(2, 1, 2)
    with pytest.raises(RuntimeError, match="row must be a CUDA tensor"):
        ops.gatv2_attention_forward(i, i, i, i, f, f, a)
    with pytest.raises(RuntimeError, match="row must be a CUDA tensor"):
        ops.gatv2_attention_backward(i, i, i, i, i, i, i, i, f, f, a, f, st, f, 0.2)
    with pytest.raises(RuntimeError, match="no CPU implementation|must be a CUDA tensor"):
        torch.ops.graphop.gatv2_attention_forward(i, i, i, i, f, f, a)
    with pytest.raises(RuntimeError, match="no CPU implementation|must be a CUDA tensor"):
        torch.ops.graphop.gatv2_attention_backward(i, i, i, i, i, i, i, i, f, f, a, f, st, f, 0.1)


def test_fused_gatv2_fast_kernels_do_not_spill():
    """Every fast instantiation keeps its loop in registers: no spill, no scratch.  9 (h, d) pairs of the forward and of
    the pack, 9 x {owned, shared} of the row and the column pass, and the kernel that sums the row pass's datt partials."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources()
    fwd = {n: r for n, r in res.items() if re.search(r"k_gv2attn_fwd_f32<\d+, \d+>\(", n)}
    pack = {n: r for n, r in res.items() if re.search(r"k_gv2attn_pack_f32<\d+, \d+>\(", n)}
    row = {n: r for n, r in res.items() if re.search(r"k_gv2attn_bwd_row_f32<\d+, \d+, (true|false)>\(", n)}
    col = {n: r for n, r in res.items() if re.search(r"k_gv2attn_bwd_col_f32<\d+, \d+, (true|false)>\(", n)}
    fin = {n: r for n, r in res.items() if re.search(r"k_gv2attn_datt_fin_f32\(", n)}
    assert (len(fwd), len(pack), len(row), len(col), len(fin)) == (9, 9, 18, 18, 1), sorted(res)
    for h, d in R.FAST:
        assert any("k_gv2attn_fwd_f32<%d, %d>(" % (h, d) in n for n in fwd), (h, d)
        assert any("k_gv2attn_pack_f32<%d, %d>(" % (h, d) in n for n in pack), (h, d)
        for owned in ("true", "false"):
            assert any("k_gv2attn_bwd_row_f32<%d, %d, %s>(" % (h, d, owned) in n for n in row), (h, d, owned)
            assert any("k_gv2attn_bwd_col_f32<%d, %d, %s>(" % (h, d, owned) in n for n in col), (h, d, owned)
    fast = {**fwd, **pack, **row, **col, **fin}
    assert len(fast) == len([n for n in res if "k_gv2attn_" in n and "_generic" not in n])   # no fast kernel left out
    bad = {n: r for n, r in fast.items() if r["spill_vgpr"] or r["spill_sgpr"] or r["scratch"]}
    assert not bad, "\n".join("%s: %r" % kv for kv in sorted(bad.items()))
    # the forward's merge of a long segment stays within 16 KB + 1 KB of LDS at the widest rows
    assert max(r["lds"] for r in fwd.values()) <= 17 * 1024


def _small_case():
    """23 x 17 nodes, h = 3, d = 5: rows 0, 5, 10, ... empty, xr = -xl on shared ids with an edge (i, i) for each (z == 0
    exactly in every component there), and row 1 with scores near 50."""
    gen = torch.Generator().manual_seed(3)
    n_l, n_r, h, d = 23, 17, 3, 5
    src = torch.randint(0, n_l, (160,), generator=gen)
    src = src[src % 5 != 0]
    dst = torch.randint(0, n_r, (src.numel(),), generator=gen)
    xl = torch.randint(-3, 4, (n_l, h, d), generator=gen).double()
    xr = torch.randint(-3, 4, (n_r, h, d), generator=gen).double()
    xr[:n_r] = -xl[:n_r]
    keep = torch.arange(n_r)
    keep = keep[keep % 5 != 0]
    src, dst = torch.cat([src, keep]), torch.cat([dst, keep])
    att = torch.randn(h, d, generator=gen, dtype=torch.float64)
    xl[1] += 12.0 * att.sign()                   # row 1: every component of z well above 0, s ~ 12 * sum |att| ~ 50
    dO = torch.randn(n_l, h, d, generator=gen, dtype=torch.float64)
    return src, dst, n_l, xl, xr, att, dO


@pytest.mark.parametrize("slope", [0.2, 0.0, -0.1])
def test_fused_gatv2_backward_formulas_match_autograd(slope):
    """stats, o, D, da, ds and the three sums as include/graphop_hip.h states them, in float64, against autograd through
    gatv2_reference.gatv2_layer(..., V=None): small rectangular graph with empty rows, exact z == 0 ties (which take the
    slope) and a row with |s| ~ 50."""
    src, dst, n_l, xl, xr, att, dO = _small_case()
    z = xl[src] + xr[dst]
    assert (z == 0).all(-1).all(-1).float().mean() > 0.1 and (z == 0).float().mean() > 0.1
    r = [x.clone().requires_grad_(True) for x in (xl, xr, att)]
    o_ref, s = gatv2_layer(src, dst, n_l, r[0], r[1], r[2], slope, None, with_scores=True)
    assert float(s.detach()[src == 1].abs().max()) > 40
    o_ref.backward(dO)
    o, stats, dxl, dxr, datt = R.restated(src, dst, n_l, xl, xr, att, dO, slope)
    assert not (src == 20).any() and not o[20].any() and not dxl[20].any()      # an empty row: o = 0, no gradient
    assert bool((stats[20, :, 0] == -1e9).all()) and not stats[20, :, 1].any()
    for name, got, want in (("o", o, o_ref.detach()), ("dxl", dxl, r[0].grad), ("dxr", dxr, r[1].grad),
                            ("datt", datt, r[2].grad)):
        torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-10, msg=lambda msg: name + ": " + msg)
    # the reference helper of the GPU tests (one head at a time) agrees with both
    ref = R.reference(type("G", (), dict(src=src, dst=dst, n_src=n_l))(), xl, xr, att, dO, slope)
    for name, got, want in zip(("o", "stats", "dxl", "dxr", "datt"), (o, stats, dxl, dxr, datt), ref):
        torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-10, msg=lambda msg: name + ": " + msg)


def test_fused_gatv2_fp32_reference_sits_inside_the_gpu_bounds():
    """torch's own fp32 evaluation of the reference against the float64 one on graphs of the GPU tests: o, stats, dxl and
    dxr inside rtol = 1e-4 / atol = 1e-5, datt inside 1e-6 * S.  The inputs do not strain the bounds the kernels are held
    to: an fp32 kernel that sums in another order has the rest of the bound as headroom.  (The graph with rows of up to
    5000 slots is left out: torch adds a row's terms one after the other in fp32, which no kernel here does, and that
    alone puts its datt at 1.7e-6 * S.)  Measured: o 0.27, stats 0.04, dxl 0.10, dxr 0.30 of the bound, datt 2.2e-8 * S."""
    from custom_op_benchmark_amd import graphs
    cases = [(R.irregular_graph(3), 1, 64, 0.2, "normal"), (R.irregular_graph(32), 8, 32, 0.2, "normal"),
             (R.slopes_graph(), 4, 16, -0.1, "ties"), (R.slopes_graph(), 1, 64, 0.2, "large"),
             (R.slopes_graph(), 4, 16, 0.0, "large"), (R.slopes_graph(), 3, 5, 1.0, "large"),
             (graphs.chung_lu_graph(20000, 200000, alpha=0.5, seed=1), 8, 8, 0.2, "normal")]
    worst = dict(o=0.0, stats=0.0, dxl=0.0, dxr=0.0, datt=0.0)
    for g, h, d, slope, kind in cases:
        x = R.inputs(g, h, d, seed=h * 100 + d, kind=kind, slope=slope)
        want = R.reference(g, *x, slope)
        got = R.reference(g, *x, slope, dtype=torch.float32)
        for name, a, b in zip(("o", "stats", "dxl", "dxr"), got, want):
            assert a.dtype == torch.float32
            worst[name] = max(worst[name], R.ratio(a, b))
        worst["datt"] = max(worst["datt"], R.datt_ratio(got[4], want[4], want[5]))
        print("(%d, %d) slope %g %s, E = %d: %s" % (h, d, slope, kind, g.n_edges,
                                                   ", ".join("%s %.3g" % kv for kv in worst.items())))
    print("worst: o %.3f, stats %.3f, dxl %.3f, dxr %.3f of the bound; datt %.3g * S" % (
        worst["o"], worst["stats"], worst["dxl"], worst["dxr"], worst["datt"]))
    assert max(worst[n] for n in ("o", "stats", "dxl", "dxr")) <= 1.0, worst
    assert worst["datt"] <= R.K32, worst
