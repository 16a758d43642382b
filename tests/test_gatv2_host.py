"""CPU tier of the GATv2 attention scores (graphop_gatv2_scores_*): the library and both bindings expose the op,
arguments are validated before anything touches a device, CPU tensors are refused, the fast kernels keep their loops in
registers, and the pure-torch reference the GPU tests compare against matches hand-computed numbers (including the
z == 0 tie)."""
import ctypes
import os
import re
import sys

import pytest
import torch

from conftest import ROOT
from gatv2_reference import gatv2_datt_scale, gatv2_layer, gatv2_scores

NAMES = ("gatv2_scores_forward", "gatv2_scores_backward")


def test_gatv2_symbols_resolve_in_the_library_and_the_extension():
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


def test_gatv2_argument_validation_without_gpu():
    from custom_op_benchmark_amd import _lib
    l = _lib.lib()
    n = ctypes.c_void_p(0)
    csr8 = [n] * 8
    ops8 = [n] * 8          # xl, xr, att, dy, dxl, dxr, datt, workspace
    rc = l.graphop_gatv2_scores_forward(7, n, n, n, n, n, n, n, n, 0, 0, 0, 0, 1, 4, 0.2, n, n)
    assert rc == 1 and b"dtype" in l.graphop_last_error()
    rc = l.graphop_gatv2_scores_backward(7, *csr8, *ops8, 0, 0, 0, 0, 0, 0, 1, 4, 0.2, n, n, n)
    assert rc == 1 and b"dtype" in l.graphop_last_error()
    rc = l.graphop_gatv2_scores_forward(0, n, n, n, n, n, n, n, n, -1, 0, 0, 0, 1, 4, 0.2, n, n)
    assert rc == 1 and b"negative" in l.graphop_last_error()
    rc = l.graphop_gatv2_scores_backward(1, *csr8, *ops8, 0, 0, 0, 0, -3, 0, 1, 4, 0.2, n, n, n)
    assert rc == 1 and b"negative" in l.graphop_last_error()
    rc = l.graphop_gatv2_scores_backward(0, *csr8, *ops8, 0, 0, 0, 0, 0, 0, 0, 4, 0.2, n, n, n)
    assert rc == 1 and b"negative" in l.graphop_last_error()          # h = 0
    rc = l.graphop_gatv2_scores_forward(0, n, n, n, n, n, n, n, n, 0, 0, 0, 0, 1, 0, 0.2, n, n)
    assert rc == 1 and b"negative" in l.graphop_last_error()          # d = 0
    # a workspace below the documented minimum, min(ceil(n_row_chunks / 16), 8192) * h * d values, is refused
    rc = l.graphop_gatv2_scores_backward(0, *csr8, *ops8, 4 * 7 * 8 - 1, 100, 0, 10, 5, 5, 2, 4, 0.2, n, n, n)
    assert rc == 1 and b"workspace" in l.graphop_last_error()
    # empty problems are no-ops that never dereference anything
    assert l.graphop_gatv2_scores_forward(0, n, n, n, n, n, n, n, n, 0, 0, 0, 0, 1, 64, 0.2, n, n) == 0
    assert l.graphop_gatv2_scores_forward(1, n, n, n, n, n, n, n, n, 0, 0, 0, 0, 4, 7, -0.1, n, n) == 0
    assert l.graphop_gatv2_scores_backward(0, *csr8, *ops8, 0, 0, 0, 0, 0, 0, 1, 64, 0.2, n, n, n) == 0
    assert l.graphop_gatv2_scores_backward(1, *csr8, *ops8, 0, 0, 0, 0, 0, 0, 8, 16, 0.0, n, n, n) == 0


def test_gatv2_cpu_tensors_are_refused():
    from custom_op_benchmark_amd import graphop as ops
    i = torch.zeros(2, dtype=torch.int64)
    f = torch.zeros(2, 4)
    a = torch.zeros(4)
    with pytest.raises(RuntimeError, match="row must be a CUDA tensor"):
        ops.gatv2_scores_forward(i, i, i, i, f, f, a)
    with pytest.raises(RuntimeError, match="row must be a CUDA tensor"):
        ops.gatv2_scores_backward(i, i, i, i, i, i, i, i, f, f, a, f[:, 0].contiguous(), 0.2)
    with pytest.raises(RuntimeError, match="no CPU implementation|must be a CUDA tensor"):
        torch.ops.graphop.gatv2_scores_forward(i, i, i, i, f, f, a)
    with pytest.raises(RuntimeError, match="no CPU implementation|must be a CUDA tensor"):
        torch.ops.graphop.gatv2_scores_backward(i, i, i, i, i, i, i, i, f, f, a, f[:, 0].contiguous(), 0.1)


def test_gatv2_ops_are_extra_ops_with_an_autograd_class():
    from custom_op_benchmark_amd import functions, graphop as ops
    for n in NAMES:
        assert n in ops.EXTRA_OPS and callable(getattr(ops, n))
        assert "float negative_slope=0.2" in ops._SCHEMAS[n] and "Tensor att" in ops._SCHEMAS[n]
    assert issubclass(functions.GATv2Scores, torch.autograd.Function)
    assert callable(functions.gatv2_attention_step)
    assert len(ops.__all__) == 8 and not set(NAMES) & set(ops.__all__)      # the reference's eight names only
    # the workspace the bindings hand to the C ABI is the header's minimum
    assert [ops._gatv2_workspace_values(c, 2, 32) for c in (0, 1, 16, 17, 16 * 8192, 10 ** 7)] == \
        [0, 64, 64, 128, 8192 * 64, 8192 * 64]


def test_gatv2_schemas_of_the_extension_equal_the_python_ones():
    from custom_op_benchmark_amd import graphop as ops
    assert ops.cpp_ext is not None, "graphop_cpp.so not built (run __graft_entry__.build())"
    for n in NAMES:
        assert torch._C.parse_schema("graphop::" + n + ops._SCHEMAS[n]) == getattr(torch.ops.graphop, n).default._schema
        assert all(torch._C._dispatch_has_kernel_for_dispatch_key("graphop::" + n, k)
                   for k in ("CUDA", "CPU"))                           # the CUDA key and the refusing CPU key


def test_gatv2_reference_matches_hand_computed_numbers():
    """4 nodes, 5 edges, d = 2, att = (2, -1), slope 0.2; edges (0, 1) and (3, 3) have z == 0 in both components and
    edge (2, 0) in the second: 0 forward, the slope backward."""
    src = torch.tensor([0, 0, 1, 2, 3])
    dst = torch.tensor([1, 2, 3, 0, 3])
    xl = torch.tensor([[1.0, 0.0], [-2.0, 1.0], [0.5, -1.0], [0.0, 2.0]], dtype=torch.float64, requires_grad=True)
    xr = torch.tensor([[3.0, 1.0], [-1.0, 0.0], [2.0, -3.0], [0.0, -2.0]], dtype=torch.float64, requires_grad=True)
    att = torch.tensor([2.0, -1.0], dtype=torch.float64, requires_grad=True)
    z = (xl[src] + xr[dst]).detach()
    assert z.tolist() == [[0.0, 0.0], [3.0, -3.0], [-2.0, -1.0], [3.5, 0.0], [0.0, 0.0]]
    y = gatv2_scores(src, dst, xl, xr, att, 0.2)
    assert y.shape == (5,) and y[0] == 0 and y[4] == 0
    assert torch.allclose(y.detach(), torch.tensor([0.0, 6.6, -0.6, 7.0, 0.0], dtype=torch.float64), rtol=0, atol=1e-14)
    dy = torch.ones(5, dtype=torch.float64)
    y.backward(dy)
    t = lambda rows: torch.tensor(rows, dtype=torch.float64)
    # g[e, c] = att[c] * (z > 0 ? 1 : 0.2): (0.4, -0.2) where both components take the slope, (2, -0.2) for edges 1 and 3
    assert torch.allclose(xl.grad, t([[2.4, -0.4], [0.4, -0.2], [2.0, -0.2], [0.4, -0.2]]), rtol=0, atol=1e-15)
    assert torch.allclose(xr.grad, t([[2.0, -0.2], [0.4, -0.2], [2.0, -0.2], [0.8, -0.4]]), rtol=0, atol=1e-15)
    assert torch.allclose(att.grad, t([0 + 3 - 0.4 + 3.5 + 0, 0 - 0.6 - 0.2 + 0 + 0]), rtol=0, atol=1e-15)
    S = gatv2_datt_scale(src, dst, xl.detach(), xr.detach(), dy, 0.2)
    assert torch.allclose(S, t([3 + 0.4 + 3.5, 0.6 + 0.2]), rtol=0, atol=1e-15)
    # several heads: every head is the one-head formula on its slice
    xl3, xr3 = torch.stack([xl, 2 * xl], 1).detach(), torch.stack([xr, -xr], 1).detach()
    att3 = torch.stack([att, att.flip(0)]).detach()
    y3 = gatv2_scores(src, dst, xl3, xr3, att3, 0.2)
    assert y3.shape == (5, 2) and torch.equal(y3[:, 0], y.detach())
    assert torch.equal(y3[:, 1], gatv2_scores(src, dst, xl3[:, 1], xr3[:, 1], att3[1], 0.2))
    # the layer: row 0 has scores (0, 6.6) over V[1], V[2]; rows 1, 2, 3 have one edge each; V=None aggregates xr
    V = torch.arange(8, dtype=torch.float64).view(4, 2)
    o = gatv2_layer(src, dst, 4, xl.detach(), xr.detach(), att.detach(), 0.2, V)
    w = torch.softmax(torch.tensor([0.0, 6.6], dtype=torch.float64), 0)
    assert torch.allclose(o[0], w[0] * V[1] + w[1] * V[2])
    assert torch.equal(o[1], V[3]) and torch.equal(o[2], V[0]) and torch.equal(o[3], V[3])
    o2 = gatv2_layer(src, dst, 4, xl.detach(), xr.detach(), att.detach(), 0.2)
    assert torch.allclose(o2[0], w[0] * xr[1] + w[1] * xr[2]) and torch.equal(o2[2], xr[0].detach())


def test_gatv2_fast_kernels_do_not_spill():
    """Every fast instantiation keeps its loop in registers: no spill, no scratch.  9 (h, d) pairs of the forward,
    9 x {owned, shared} of the row and the column pass, and the kernel that sums the row pass's datt partials."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources()
    fwd = {n: r for n, r in res.items() if re.search(r"k_gatv2_fwd_f32<\d+, \d+>\(", n)}
    row = {n: r for n, r in res.items() if re.search(r"k_gatv2_bwd_row_f32<\d+, \d+, (true|false)>\(", n)}
    col = {n: r for n, r in res.items() if re.search(r"k_gatv2_bwd_col_f32<\d+, \d+, (true|false)>\(", n)}
    fin = {n: r for n, r in res.items() if re.search(r"k_gatv2_datt_fin_f32\(", n)}
    assert (len(fwd), len(row), len(col), len(fin)) == (9, 18, 18, 1), sorted(res)
    fast = {**fwd, **row, **col, **fin}
    assert len(fast) == len([n for n in res if "k_gatv2_" in n and "_generic" not in n])   # no fast kernel left out
    bad = {n: r for n, r in fast.items() if r["spill_vgpr"] or r["spill_sgpr"] or r["scratch"]}
    assert not bad, "\n".join("%s: %r" % kv for kv in sorted(bad.items()))
    # the row pass is compiled for four workgroups per CU
    assert all(r["vgpr"] <= 128 for r in row.values()), row
    generic = [n for n in res if re.search(r"k_gatv2_(fwd|bwd_row|bwd_col)_generic<(float|double)>\(", n)]
    assert len(generic) == 6, generic
