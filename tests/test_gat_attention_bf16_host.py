"""CPU tier of the fused GAT layer on bfloat16 tables (kernels_gat_attn_bf16.h): the float64 reference
against autograd, the three new symbols under ABI 8, the stated workspace sums, each named refusal, the old entry points'
answer to dtype 2, and a gfx950 code object without scratch.  Plans are the stand-ins of test_attention_bf16_host.py."""
import ctypes
import os
import re
import sys

import pytest
import torch

import gat_bf16_reference as R
from dropout_reference import gat_layer_dropout, multipliers
from test_attention_bf16_host import _plan, lib          # noqa: F401 (fixture)
from test_attention_heads_host import _up
from util import random_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD = [(1, 64), (2, 32), (2, 64), (4, 16), (4, 32), (4, 64), (8, 8), (8, 16), (8, 32)]
NULL, SOME = ctypes.c_void_p(0), ctypes.c_void_p(4096)


def _seg_plan(*args, **kw):
    plan = _plan(*args, **kw)
    plan.seg_chunk = 256          # (never read on the host)
    return plan


def _query(l, backward, C_r, C_c, E, n_l, n_r, h, d, pr, pc):
    out = ctypes.c_int64(-1)
    assert l.graphop_gat_attention_bf16_workspace_bytes(backward, C_r, C_c, E, n_l, n_r, h, d, ctypes.byref(pr) if pr else NULL,
                                                        ctypes.byref(pc) if pc else NULL, ctypes.byref(out)) == 0
    return out.value


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_reference_backward_is_autograd_of_the_layer(p):
    g = random_graph(40, 47, 300, seed=1, chunk_size=4, zero_rows=0.2, hub=30)
    gen = torch.Generator().manual_seed(2)
    h, d = 4, 8
    el, er, V, dO = (torch.randn(s, generator=gen, dtype=torch.float64)
                     for s in ((g.n_src, h), (g.n_dst, h), (g.n_dst, h, d), (g.n_src, h, d)))
    mult = multipliers(g.src.numpy(), g.dst.numpy(), h, p, 11, 3) if p else None
    leaves = [x.clone().requires_grad_(True) for x in (el, er, V)]
    o = gat_layer_dropout(g.src, g.dst, g.n_src, *leaves, -0.3, p, 11, 3)
    o.backward(dO)
    o0, m0, linv0 = R.forward(g.src, g.dst, g.n_src, el, er, V, -0.3, mult)
    torch.testing.assert_close(o0, o.detach(), rtol=1e-12, atol=1e-12)
    empty = torch.bincount(g.src, minlength=g.n_src) == 0
    assert empty.any() and bool((m0[empty] == -1e9).all()) and not linv0[empty].any()
    for x, leaf in zip(R.backward(g.src, g.dst, el, er, V, o.detach(), dO, -0.3, mult), leaves):
        torch.testing.assert_close(x, leaf.grad, rtol=1e-11, atol=1e-12)


def test_abi_symbols_and_routing(lib):          # noqa: F811
    from custom_op_benchmark_amd import _lib
    assert _lib.ABI_VERSION == 8 and lib.graphop_abi_version() == 8
    for name in ("workspace_bytes", "forward", "backward"):
        assert hasattr(lib, "graphop_gat_attention_bf16_" + name)
    x = torch.zeros(2, dtype=torch.bfloat16)
    assert all(_lib.gat_attn_is_bf16("gat_attention" + f, x) for f in ("_forward", "_backward", "_dropout_forward",
                                                                       "_dropout_backward"))
    assert not _lib.gat_attn_is_bf16("gat_edge_attention_forward", x) and not _lib.gat_attn_is_bf16("gat_attention_forward", x.float())


def test_workspace_queries_answer_the_stated_sums(lib):          # noqa: F811
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    E, n_l, n_r = 400000, 50, 40
    for C_r, C_c in ((100, 107), (3 * n_cu * 64 + 5, 2 * n_cu * 64 + 1)):          # one, and three / two chunks per group
        cpg = [min(16, max(1, C // (n_cu * 16 * 4))) for C in (C_r, C_c)]
        assert cpg == ([1, 1] if C_r == 100 else [3, 2])
        np_r, np_c = (2 * -(-C // k) for C, k in zip((C_r, C_c), cpg))
        pr, pc = _seg_plan(C_r, E, n_l - 1, n_r - 1), _seg_plan(C_c, E, n_r - 1, n_l - 1)
        for h, d in ((8, 8), (4, 64)):
            F, np_m = h * d, max(np_r, np_c)
            fwd = _up(4 * n_l * h) + _up(4 * n_r * h) + _up(4 * np_r) + _up(4 * np_r * F)
            bwd = _up(16 * n_l * h) + _up(4 * np_m) + _up(4 * h * np_m) + _up(4 * F * np_c)
            assert _query(lib, 0, C_r, 0, E, n_l, n_r, h, d, pr, None) == fwd, (h, d, C_r)
            assert _query(lib, 1, C_r, C_c, E, n_l, n_r, h, d, pr, pc) == bwd, (h, d, C_r)
    # 0 where the op refuses: a pair outside the set, no plan, an unsorted chunk list, a plan without neighbour ids,
    # id ranges outside the tables; and where there is nothing to do
    assert _query(lib, 0, 100, 0, E, n_l, n_r, 3, 8, pr, None) == _query(lib, 1, C_r, C_c, E, n_l, n_r, 8, 64, pr, pc) == 0
    assert _query(lib, 0, C_r, 0, E, n_l, n_r, 4, 16, None, None) == _query(lib, 1, C_r, C_c, E, n_l, n_r, 4, 16, pr, None) == 0
    for bad in (_seg_plan(C_r, E, n_l - 1, n_r - 1, row_owned=0), _seg_plan(C_r, E, n_l - 1, n_r - 1, indices=False),
                _seg_plan(C_r, E, n_l, n_r - 1), _seg_plan(C_r, E, n_l - 1, n_r)):
        assert _query(lib, 0, C_r, 0, E, n_l, n_r, 4, 16, bad, None) == 0
    assert _query(lib, 0, 0, 0, 0, n_l, n_r, 4, 16, _seg_plan(0, 0, -1, -1), None) == 0


def _forward(l, h, d, plan, V=SOME, ws_bytes=1 << 30, C=4, E=10):
    return l.graphop_gat_attention_bf16_forward(SOME, SOME, SOME, SOME, SOME, SOME, V, SOME, SOME, SOME, ws_bytes, C, E, 5, 5,
                                                h, d, 0.2, 0.5, 1, 0, ctypes.byref(plan) if plan else NULL, NULL)


def test_refusals_are_named_and_the_old_entry_points_keep_theirs(lib):          # noqa: F811
    plan = _seg_plan(4, 10, 4, 4)
    for f in (plan.row, plan.indptr, plan.eid):          # the plan of the call's arrays
        assert f is None
    plan.row = plan.indptr = plan.eid = plan.indices = 4096
    assert _forward(lib, 3, 8, plan) == 1
    assert b"gat_attention_bf16_forward: bfloat16 unsupported: (h, d) = (3, 8) is not in the bfloat16 set" in lib.graphop_last_error()
    assert _forward(lib, 4, 16, None) == 1
    assert b"bfloat16 unsupported: plan is NULL" in lib.graphop_last_error()
    assert _forward(lib, 4, 16, plan, V=ctypes.c_void_p(4096 + 8)) == 1
    assert b"bfloat16 tables must be 16-byte aligned" in lib.graphop_last_error()
    assert _forward(lib, 4, 16, plan, ws_bytes=16) == 1
    assert b"graphop_gat_attention_bf16_workspace_bytes" in lib.graphop_last_error()
    n, some = NULL, SOME
    assert lib.graphop_gat_attention_bf16_backward(*([some] * 18), 1 << 30, 4, 4, 10, 5, 5, 4, 16, 0.2, 0.0, 0, 0,
                                                   ctypes.byref(plan), n, n) == 1
    assert b"gat_attention_bf16_backward: bfloat16 unsupported: plan_c is NULL" in lib.graphop_last_error()
    # dtype 2 at the entry points that take a dtype: refused as before
    assert lib.graphop_gat_attention_forward(2, *([some] * 9), 4, 10, 5, 5, 4, 16, 0.2, n, n) == 1
    assert b"gat_attention_forward: dtype must be GRAPHOP_F32 or GRAPHOP_F64" in lib.graphop_last_error()
    assert lib.graphop_gat_attention_dropout_backward(2, *([some] * 18), 0, 4, 4, 10, 5, 5, 4, 16, 0.2, 0.5, 1, 0, n, n, n) == 1
    assert b"gat_attention_dropout_backward: dtype must be" in lib.graphop_last_error()


def test_gat_bf16_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    fam = {}
    for name, r in kernel_resources().items():
        m = re.search(r"graphop::(k_gat_attn_bf16_\w+)<(.*)>\(", name)
        if m:
            assert not r["spill_vgpr"] and not r["scratch"] and r["vgpr"] <= 256, (name, r)
            fam.setdefault(m.group(1), set()).add(m.group(2))
    hd = {"%d, %d" % x for x in HD}
    both = {a + ", " + b for a in hd for b in ("false", "true")}
    assert fam == {"k_gat_attn_bf16_fwd": both, "k_gat_attn_bf16_fwd_merge": hd, "k_gat_attn_bf16_pack": hd,
                   "k_gat_attn_bf16_bwd_row": both, "k_gat_attn_bf16_bwd_col": both, "k_gat_attn_bf16_bwd_merge": both}
