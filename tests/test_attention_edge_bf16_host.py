"""CPU tier of the bfloat16 fused attention step with edge features (kernels_attn_edge_bf16.h): empty
problems touch nothing, every refusal is named, the workspace is the plain bf16 step's, the ops are bound and not
registered, and the set of k_edge_bf16_* instantiations is exact, out of scratch and within 256 VGPRs."""
import ctypes
import os
import re
import sys

import torch

from test_attention_bf16_host import HD, _plan, lib          # noqa: F401 (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SOME = ctypes.c_void_p(0), ctypes.c_void_p(4096)


def _fwd(lib, h, d, plan=NULL, ptr=SOME, sizes=(4, 10, 5, 5), p=0.5, head0=0, xe=None):          # noqa: F811
    ptrs = [ptr] * 7 + [ptr if xe is None else xe] + [ptr] * 2
    return lib.graphop_attention_edge_bf16_forward(*ptrs, *sizes, h, d, NULL, 0, plan, NULL, p, 1, 0, head0)


def _bwd(lib, h, d, ptrs, sizes, plans=(NULL, NULL)):          # noqa: F811
    return lib.graphop_attention_edge_bf16_backward(*ptrs, *sizes, h, d, NULL, 0, *plans, NULL, 0.5, 1, 0, 0)


def test_empty_problems_touch_nothing_and_refusals_are_named(lib):          # noqa: F811
    from custom_op_benchmark_amd import _lib
    assert _lib.ABI_VERSION == 8 and lib.graphop_abi_version() == 8
    for h, d in ((4, 16), (8, 64)):
        assert _fwd(lib, h, d, ptr=NULL, sizes=(0, 0, 0, 7)) == 0
        assert _bwd(lib, h, d, [NULL] * 19, (0, 0, 0, 0, 0)) == 0
    E, C, n_q, n_k = 1000, 100, 50, 40
    pr, pc = _plan(C, E, n_q - 1, n_k - 1), _plan(C + 7, E, n_k - 1, n_q - 1)
    for kw, message in ((dict(), b"attention_edge_bf16_forward: bfloat16 unsupported: plan is NULL"),
                        (dict(h=3, d=8), b"(h, d) = (3, 8) is not in the bfloat16 set"),
                        (dict(p=1.0), b"dropout probability p must be in [0, 1)"),
                        (dict(head0=-1), b"head0 >= 0 and head0 + h < 2^31 wanted"),
                        (dict(xe=NULL), b"attention_edge_bf16_forward: xe is NULL")):
        assert _fwd(lib, kw.pop("h", 4), kw.pop("d", 16), **kw) == 1
        assert message in lib.graphop_last_error(), lib.graphop_last_error()
    assert _bwd(lib, 4, 16, [SOME] * 19, (4, 4, 10, 5, 5)) == 1
    assert b"attention_edge_bf16_backward: bfloat16 unsupported: plan_r is NULL" in lib.graphop_last_error()
    # the query equals the plain bf16 step's in both directions, and answers 0 where a call would refuse
    out, plain = ctypes.c_int64(-1), ctypes.c_int64(-1)
    query = lambda backward, h, d, a, b: lib.graphop_attention_edge_bf16_workspace_bytes(
        backward, E, n_q, n_k, h, d, a, b, NULL, ctypes.byref(out))
    for backward in (0, 1):
        assert lib.graphop_attention_bf16_opts_workspace_bytes(backward, E, n_q, n_k, 4, 16, ctypes.byref(pr), ctypes.byref(pc),
                                                               NULL, 0, ctypes.byref(plain)) == 0
        assert query(backward, 4, 16, ctypes.byref(pr), ctypes.byref(pc)) == 0 and out.value == plain.value > 0
        assert query(backward, 3, 8, ctypes.byref(pr), ctypes.byref(pc)) == 0 and out.value == 0
        assert query(backward, 4, 16, NULL, NULL) == 0 and out.value == 0
    unowned = _plan(C, E, n_q - 1, n_k - 1, row_owned=0)
    assert query(0, 4, 16, ctypes.byref(unowned), NULL) == 0 and out.value == 0


def test_ops_are_bound_and_not_registered():
    from custom_op_benchmark_amd import graphop
    for name in ("attention_edge_bf16_forward", "attention_edge_bf16_backward"):
        assert name in graphop.EXTRA_OPS and name not in graphop._SCHEMAS and callable(getattr(graphop, name))
        assert not hasattr(torch.ops.graphop, name)


def test_instantiation_set_is_exact_and_out_of_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    fam = {}
    for name, r in kernel_resources().items():
        m = re.search(r"graphop::(k_edge_bf16_\w+)<(.*)>\(", name)
        if m:
            assert not r["spill_vgpr"] and not r["scratch"] and r["vgpr"] <= 256, (name, r)
            fam.setdefault(m.group(1), set()).add(m.group(2))
    hd = ["%d, %d" % x for x in HD]
    tf = ("false", "true")
    fwd = {"%s, %s" % (a, drop) for a in hd for drop in tf}
    bwd = {"%s, %s, %s" % (a, col, drop) for a in hd for col in tf for drop in tf}
    assert fam == {"k_edge_bf16_fwd_rows": fwd, "k_edge_bf16_bwd_rows": bwd}
